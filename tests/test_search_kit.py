"""The shared helpers of the search tests (search_kit.py) reject what they are there to reject.  No GPU: the row helpers run on
host buffers."""
import numpy as np
import pytest
import torch

import search_kit as K
from fira_icse_amd import _lib
from fira_icse_amd.config import FiraConfig


def search_result(p=(0.5, 0.25)):
    """(gen [2, 5], length [2], prob [2]) of a greedy search: the ids past a length are junk."""
    gen = torch.tensor([[2, 7, 8, 1, 99], [2, 9, 1, 98, 97]])
    return gen, torch.tensor([4, 3]), torch.tensor(p, dtype=torch.float32)


def test_same_search_passes_when_ids_differ_only_beyond_the_lengths():
    gen, length, p = search_result()
    other = gen.clone()
    other[0, 4], other[1, 3:] = 5, 6
    K.same_search((gen, length, p), (other, length, p))
    K.same_search((gen, length, p, "a fourth element is ignored"), (other, length, p))
    beam = tuple(t[None].expand(3, *t.shape).contiguous() for t in (gen, length, p))        # [B, beam, T] shapes too
    K.same_search(beam, (other[None].expand(3, 2, 5).contiguous(), beam[1], beam[2]))


def test_same_search_raises_when_an_id_inside_a_length_differs():
    gen, length, p = search_result()
    for at in ((0, 3), (1, 2), (0, 0)):                       # the last id inside each length, and the first
        other = gen.clone()
        other[at] += 1
        with pytest.raises(AssertionError):
            K.same_search((gen, length, p), (other, length, p))


def test_same_search_raises_when_a_length_differs():
    gen, length, p = search_result()
    with pytest.raises(AssertionError):
        K.same_search((gen, length, p), (gen, torch.tensor([4, 2]), p))


def test_same_search_raises_when_a_probability_differs_by_one_ulp():
    gen, length, p = search_result()
    ulp = torch.from_numpy(np.nextafter(p.numpy(), np.float32(1.0)))
    assert float((ulp - p).abs().max()) <= 2.0 ** -24
    with pytest.raises(AssertionError):
        K.same_search((gen, length, p), (gen, length, ulp))
    zero = search_result((0.5, 0.0))[2]                       # and by the sign of a zero
    with pytest.raises(AssertionError):
        K.same_search((gen, length, zero), (gen, length, -zero))


def test_bits_tells_the_zeros_and_two_nan_payloads_apart():
    plus, minus = np.array([0.0], dtype=np.float32), np.array([-0.0], dtype=np.float32)
    assert plus == minus and not torch.equal(K.bits(plus), K.bits(minus))
    nans = np.array([0x7FC00000, 0x7FC00001], dtype=np.uint32).view(np.float32)
    assert np.isnan(nans).all()
    assert not torch.equal(K.bits(nans[:1]), K.bits(nans[1:])) and torch.equal(K.bits(nans[:1]), K.bits(nans[:1].copy()))
    assert torch.equal(K.bits(torch.from_numpy(plus)), K.bits(plus)) and K.bits(plus).dtype == torch.int32


W45 = 37 + 5 + 3                                                    # the SMALL geometry of the edit-kernel tests


def test_offset_rows_begin_at_every_alignment_and_outside_untouched_guards_both_sides():
    values = np.arange(1, 7 * W45 + 1, dtype=np.float32).reshape(7, W45)
    starts = set()
    for offset in range(4):
        buf, view = K.offset_rows(values, offset, device="cpu")
        assert buf.numel() == values.size + offset + K.PAD_FLOATS and torch.equal(view, torch.from_numpy(values))
        assert view.data_ptr() - buf.data_ptr() == 4 * offset
        starts |= {(4 * (offset + r * W45)) % 16 for r in range(7)}
        assert [(view[r].data_ptr() - buf.data_ptr()) % 16 for r in range(4)] == [(4 * (offset + r * W45)) % 16 for r in range(4)]
        assert K.outside_untouched(buf, offset, values.size)
        view.fill_(9.0)                                             # writes inside the rows are not its business
        assert K.outside_untouched(buf, offset, values.size)
        for at in ([offset - 1] if offset else []) + [offset + values.size, buf.numel() - 1]:   # just before, just after, the end
            buf[at] = 1e-30
            with pytest.raises(AssertionError):
                K.outside_untouched(buf, offset, values.size)
            buf[at] = 0.0
    assert starts == {0, 4, 8, 12}
    buf, view = K.offset_rows(values, 1, fill=-3.0, device="cpu")   # a sentinel instead of 0: a stray 0 is a write too
    assert K.outside_untouched(buf, 1, values.size, fill=-3.0)
    buf[0] = 0.0
    with pytest.raises(AssertionError):
        K.outside_untouched(buf, 1, values.size, fill=-3.0)


def test_device_dims_sets_the_four_fields_and_leaves_the_others():
    base, d = _lib.make_dims(FiraConfig()), K.device_dims(37, 5, 3, 8)
    assert (d.vocab, d.sou_len, d.sub_len, d.tar_len) == (37, 5, 3, 8)
    four = {"vocab", "sou_len", "sub_len", "tar_len"}
    others = [name for name, _ in d._fields_ if name not in four]
    assert others and all(getattr(d, name) == getattr(base, name) for name in others)
    d = K.device_dims(sub_len=0)                                    # a field that is not given keeps the configuration's value
    assert d.sub_len == 0 and (d.vocab, d.sou_len, d.tar_len) == (base.vocab, base.sou_len, base.tar_len)
    assert K.dims_of(FiraConfig()) == (base.vocab, base.sou_len, base.sub_len)


def test_counting_lib_counts_and_forwards():
    class Real:
        def fira_twice(self, x):
            return 2 * x
    lib = K.CountingLib(Real())
    assert lib.fira_twice(21) == 42 and lib.fira_twice(1) == 2
    assert lib.calls == {"fira_twice": 2}
    with pytest.raises(AttributeError):
        lib.fira_missing
