// Teacher-forced scoring of a given next word against the decode step's output distribution.
//
// One workgroup of 1024 threads per (commit, candidate) row, in the register-resident form of decode_dist_wide_kernel
// (copyhead.hip) and sample_dist_kernel (sample.hip): the row's V generator logits are requested once and stay in registers
// (25 per thread), the S <= 1024 copy slots are one per thread.  The kernel forms the same distribution p over V + S entries
// with the same arithmetic in the same order, so the optional `dist` row and every single-entry probability reported here are
// bit-identical to what fira_decode_step writes.  Then, for the row's target word y (a vocabulary id, 0 = nothing to score):
//   p_word      p[y] (y < V) + sum of p[V + s] over the VALID memory slots s whose source id (sou[b, s] below L, sub_token[b, s - L]
//               above) is y: the probability that the model emits the WORD, whichever entry it takes.  The copy part is one
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
    const rsrc_t rL = buf_rsrc(logits + (size_t)r * ldl, (unsigned)V * 4u);
    float x[DDW_NPT];
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) x[i] = buf_load_f32(rL, (unsigned)(tid + DDW_NT * i) * 4u);   // past V: 0, replaced below
    const int b = r / n_cand;
    const float* srow = score + (size_t)r * S;
    const int32_t* mv = mem_valid + (size_t)b * S;
    const int y = target[r];
    const int lab = label ? label[r] : -1;
    const int valid = tid < S ? mv[tid] : 0;
    // the word this thread's memory slot copies (requested here, used after the distribution is formed)
    int src = 0;
    if (tid < L) src = sou[(size_t)b * L + tid];
    else if (tid < S) src = sub[(size_t)b * (S - L) + (tid - L)];
    // ---- the distribution: decode_dist_wide_kernel's arithmetic, operation for operation
    float z0, z1;
    {                                                          // gate = x wp^T + bp: two 256-long dot products
        const float xv = tid < FIRA_D ? xrow[(size_t)r * FIRA_D + tid] : 0.f;
        const float a0 = tid < FIRA_D ? xv * wp[tid] : 0.f, a1 = tid < FIRA_D ? xv * wp[FIRA_D + tid] : 0.f;
        z0 = block16_sum(a0, smf) + bp[0];
        z1 = block16_sum(a1, smf) + bp[1];
    }
    const float zm = fmaxf(z0, z1);
    const float e0 = expf(z0 - zm), e1 = expf(z1 - zm);
    const float g0 = e0 / (e0 + e1), g1 = e1 / (e0 + e1);
    float cmax = -INFINITY, gmax = -INFINITY;
    int cidx = 0x7fffffff, gidx = 0x7fffffff;
    const float sv = tid < S ? (valid ? srow[tid] : -1e9f) : -INFINITY;         // S <= 1024: one slot per thread
    if (tid < S) { cmax = sv; cidx = tid; }
    block16_argmax(cmax, cidx, smf, smi);
    const float ce = tid < S ? expf(sv - cmax) : 0.f;
    const float csum = block16_sum(ce, smf);
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) {                      // ascending index within the thread: first maximum wins
        const int j = tid + DDW_NT * i;
        x[i] = j < V ? x[i] : -INFINITY;
        if (x[i] > gmax) { gmax = x[i]; gidx = j; }
    }
    block16_argmax(gmax, gidx, smf, smi);
    float gsum = 0.f;
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) {
        x[i] = expf(x[i] - gmax);                            // exp(-inf) = 0 past V
        gsum += x[i];
    }
    gsum = block16_sum(gsum, smf);
    const float sg = g0 * (1.0f / gsum), sc = g1 * (1.0f / csum);
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) x[i] = sg * x[i];      // p of entry tid + 1024 i
    const float pc = sc * ce;                                // p of entry V + tid
    if (dist) {
        float* drow = dist + (size_t)r * (V + S);
        const rsrc_t rD = buf_rsrc(drow, (unsigned)V * 4u);
#pragma unroll
        for (int i = 0; i < DDW_NPT; ++i)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x[i]), rD, (unsigned)(tid + DDW_NT * i) * 4u, 0, 0);
        if (tid < S) drow[V + tid] = pc;
    }
    if (tid == 0) top_id[r] = sg >= sc ? gidx : V + cidx;    // the largest entry: exp(0) = 1 times its scale
    // ---- the labelled entry: its owner reports it (no reduction)
    if (p_label) {
        const bool scored = y != 0 && lab >= 0 && lab < V + S;
        float pl = 0.f;
        bool own = !scored && tid == 0;                      // nothing to report: thread 0 writes the 0
        if (scored && lab < V) {                             // entry lab = register lab / 1024 of thread lab % 1024
            own = tid == (lab & (DDW_NT - 1));
#pragma unroll
            for (int i = 0; i < DDW_NPT; ++i) pl = (lab >> 10) == i ? x[i] : pl;       // a wave-uniform select
        } else if (scored && lab - V == tid && tid < S) {
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
    const bool hit = valid && src == y;                      // valid implies tid < S
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
    FIRA_REQUIRE(V <= DDW_NPT * DDW_NT && S <= DDW_NT,
                 "score_dist: vocabulary %d / %d memory slots exceed the register-resident row (%d / %d)", V, S,
                 DDW_NPT * DDW_NT, DDW_NT);
    hipLaunchKernelGGL(score_dist_kernel, dim3(R), dim3(DDW_NT), 0, s, V, L, S, logits, ldl, score, mem_valid, n_cand, x, wp, bp,
                       target, label, sou, sub, dist, p_word, p_entry, entry, copy_share, p_label, top_id, logp_word,
                       logp_entry, logp_label);
    FIRA_CHECK_LAUNCH("score_dist");
    return 0;
}

}  // namespace fira
