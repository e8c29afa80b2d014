// Teacher-forced scoring of a given next word against the decode step's output distribution.
//
// One workgroup of 1024 threads per (commit, candidate) row.  The row is WideRow (decode_row.h), the distribution p over V + L + S
// entries that fira_decode_step writes, so the optional `dist` row and every single-entry probability reported here have its bits.
// What this kernel adds, for the row's target word y (a vocabulary id, 0 = nothing to score):
//   p_word      p[y] (y < V) + sum of p[V + s] over the VALID memory slots s whose word (slot_word) is y: the probability that
//               the model emits the WORD, whichever entry it takes.  The copy part is one
//               block16_sum (per-thread term, the DPP tree, the 16 wave partials in order); the generator entry is added last.
//               No atomics, so every run and every graph replay gives the same bits.
//   p_entry     the largest single entry that resolves to y and its index (block16_argmax: lowest index on ties)
//   copy_share  the copy part of p_word over p_word
//   p_label     p[label] of an optional labelled entry (the entry the training loss credits)
//   top_id      the row's arg-max entry, as decode_dist_wide_kernel's best_id
// and the running sums logp_* += logf(max(p, 1e-10)) (the clamp of the training loss) of the row's message.
// A masked slot never matches: its p is exp(-1e9 - max) = 0 anyway, but a padded slot carries id 0 / stale ids.
#include "engine.h"
#include "epilogue.h"
#include "decode_row.h"

namespace fira {

__global__ __launch_bounds__(DDW_NT) void score_dist_kernel(int V, int L, int S, const float* __restrict__ logits, int ldl,
                                                            const float* __restrict__ score,
                                                            const int32_t* __restrict__ mem_valid, int n_cand,
                                                            const float* __restrict__ xrow, const float* __restrict__ wp,
                                                            const float* __restrict__ bp,
                                                            const int32_t* __restrict__ target,
                                                            const int32_t* __restrict__ label,
                                                            const int32_t* __restrict__ sou,
                                                            const int32_t* __restrict__ sub, float* __restrict__ dist,
                                                            float* __restrict__ p_word, float* __restrict__ p_entry,
                                                            int32_t* __restrict__ entry, float* __restrict__ copy_share,
                                                            float* __restrict__ p_label, int32_t* __restrict__ top_id,
                                                            float* __restrict__ logp_word, float* __restrict__ logp_entry,
                                                            float* __restrict__ logp_label) {
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    __shared__ float sm_gen;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int b = r / n_cand, NS = L + S;
    const int y = target[r];
    const int lab = label ? label[r] : -1;
    const int src = slot_word(sou, sub, (size_t)b, L, S, tid);       // (requested here, used after the distribution is formed)
    WideRow row;
    row.form(V, NS, logits + (size_t)r * ldl, score + (size_t)r * NS, mem_valid + (size_t)b * NS, r, nullptr, xrow, wp, bp, smf, smi);
    if (dist) row.store(dist + (size_t)r * (V + NS), V, NS);
    if (tid == 0) top_id[r] = row.best(V);
    const bool valid = row.valid;                            // implies tid < NS
    const float sg = row.sg;
    float(&x)[DDW_NPT] = row.x;
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) x[i] = sg * x[i];      // p of entry tid + 1024 i
    const float pc = row.sc * row.ce;                        // p of entry V + tid
    // ---- the labelled entry: its owner reports it (no reduction)
    if (p_label) {
        const bool scored = y != 0 && lab >= 0 && lab < V + NS;
        float pl = 0.f;
        bool own = !scored && tid == 0;                      // nothing to report: thread 0 writes the 0
        if (scored && lab < V) {                             // entry lab = register lab / 1024 of thread lab % 1024
            own = tid == (lab & (DDW_NT - 1));
#pragma unroll
            for (int i = 0; i < DDW_NPT; ++i) pl = (lab >> 10) == i ? x[i] : pl;       // a wave-uniform select
        } else if (scored && lab - V == tid && tid < NS) {
            pl = pc; own = true;
        }
        if (own) {
            p_label[r] = pl;
            if (scored) logp_label[r] += logf(fmaxf(pl, 1e-10f));
        }
    }
    if (y == 0) {                                            // wave-uniform (the whole row): nothing to score
        if (tid == 0) { p_word[r] = 0.f; p_entry[r] = 0.f; entry[r] = -1; copy_share[r] = 0.f; }
        return;
    }
    // ---- the entries that resolve to y: generator entry y (one thread owns it) and the valid slots that carry y
    static_assert(DDW_NT == 1024, "entry j lives in register j >> 10 of thread j & 1023");
    const bool gen_owner = tid == (y & (DDW_NT - 1));
    float gy = 0.f;
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) gy = (y >> 10) == i ? x[i] : gy;          // a wave-uniform select; y >= V: past V is 0
    gy = y < V ? gy : 0.f;
    if (gen_owner) sm_gen = gy;                              // exactly one writer; read after the barriers below
    const bool hit = valid && src == y;
    float ev = -INFINITY;
    int ei = 0x7fffffff;
    if (hit) { ev = pc; ei = V + tid; }
    if (gen_owner && y < V && gy >= ev) { ev = gy; ei = y; }     // the generator index is the lower one
    block16_argmax(ev, ei, smf, smi);
    const float copy = block16_sum(hit ? pc : 0.f, smf);
    if (tid == 0) {
        const float pw = sm_gen + copy;
        const bool any = ei != 0x7fffffff;
        const float pe = any ? ev : 0.f;
        p_word[r] = pw;
        p_entry[r] = pe;
        entry[r] = any ? ei : -1;
        copy_share[r] = pw > 0.f ? copy / pw : 0.f;
        logp_word[r] += logf(fmaxf(pw, 1e-10f));
        logp_entry[r] += logf(fmaxf(pe, 1e-10f));
    }
}

int score_dist(hipStream_t s, int R, int n_cand, int V, int L, int S, const float* logits, int ldl, const float* score,
               const int32_t* mem_valid, const float* x, const float* wp, const float* bp, const int32_t* target,
               const int32_t* label, const int32_t* sou, const int32_t* sub, float* dist, float* p_word, float* p_entry,
               int32_t* entry, float* copy_share, float* p_label, int32_t* top_id, float* logp_word, float* logp_entry,
               float* logp_label) {
    ProfScope prof(s, PROF_HEAD, 0.0);
    if (R <= 0) return 0;
    FIRA_REQUIRE(V <= ROW_MAX_V && S <= ROW_MAX_SLOTS,
                 "score_dist: vocabulary %d / %d memory slots exceed the register-resident row (%d / %d)", V, S, ROW_MAX_V,
                 ROW_MAX_SLOTS);
    // S counts all memory slots here (engine.hip passes mem_len); the kernel takes (sou_len, sub_len) like every other one
    hipLaunchKernelGGL(score_dist_kernel, dim3(R), dim3(DDW_NT), 0, s, V, L, S - L, logits, ldl, score, mem_valid, n_cand, x, wp, bp,
                       target, label, sou, sub, dist, p_word, p_entry, entry, copy_share, p_label, top_id, logp_word,
                       logp_entry, logp_label);
    FIRA_CHECK_LAUNCH("score_dist");
    return 0;
}

}  // namespace fira
