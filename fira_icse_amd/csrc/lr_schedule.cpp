// Learning-rate schedules (include/fira_hip.h: fira_lr_schedule).  fira_lr_at is the ONLY place the formulas exist: the
// dense updates are handed its value for their step, the row-sparse update's ring (AdamRowsHist::lr, copyhead.hip:
// adam_rows_hist) its value for every step a lazy row may still owe, and Python reaches it through ctypes (ops.lr_at) -- so
// every consumer divides the same float by the same bias correction.  Host code only: no device code, no HIP call.
#include "engine.h"
#include <algorithm>
#include <cmath>

extern "C" {

float fira_lr_at(const fira_lr_schedule* s, int step) {
#pragma clang fp contract(off)
    if (!s) return 0.f;
    // evaluated in double, rounded to float once (the return); no contraction: the tests compare bit for bit with the plain
    // float64 expression
    const double t = (double)std::max(step, 1), W = (double)s->warmup_steps, N = (double)s->decay_steps;
    const double base = (double)s->base_lr, mn = (double)s->min_lr;
    const double w = s->warmup_steps > 0 ? std::min(1.0, t / W) : 1.0;
    switch (s->kind) {
    case 1:                                                   // inv_sqrt
        if (s->warmup_steps < 1) return (float)base;
        return (float)(base * std::min(t / W, std::sqrt(W / t)));
    case 2:
    case 3: {
        if (t <= W) return (float)(base * w);
        const double q = N > W ? std::min(std::max((t - W) / (N - W), 0.0), 1.0) : 1.0;
        const double pi = 3.141592653589793;
        if (s->kind == 2) return (float)(mn + (base - mn) * 0.5 * (1.0 + std::cos(pi * q)));
        return (float)(mn + (base - mn) * (1.0 - q));
    }
    default:                                                  // constant
        return (float)(base * w);
    }
}

int fira_lr_schedule_check(const fira_lr_schedule* s) {
    static const char* const names[4] = {"constant", "inv_sqrt", "cosine", "linear"};
    FIRA_REQUIRE(s, "fira_lr_schedule: null schedule");
    FIRA_REQUIRE(s->kind >= 0 && s->kind <= 3, "fira_lr_schedule: kind %d is not one of 0 constant, 1 inv_sqrt, 2 cosine, 3 linear",
                 s->kind);
    FIRA_REQUIRE(std::isfinite(s->base_lr) && s->base_lr > 0.f, "fira_lr_schedule: base_lr must be finite and > 0, got %g",
                 (double)s->base_lr);
    FIRA_REQUIRE(s->warmup_steps >= 0, "fira_lr_schedule: warmup_steps must be >= 0, got %d", s->warmup_steps);
    FIRA_REQUIRE(s->kind != 1 || s->warmup_steps >= 1, "fira_lr_schedule: inv_sqrt needs warmup_steps >= 1, got %d", s->warmup_steps);
    FIRA_REQUIRE(s->kind < 2 || s->decay_steps > s->warmup_steps, "fira_lr_schedule: %s needs decay_steps > warmup_steps, got %d <= %d",
                 names[s->kind], s->decay_steps, s->warmup_steps);
    // (written so that a nan fails)
    FIRA_REQUIRE(s->min_lr >= 0.f && s->min_lr <= s->base_lr, "fira_lr_schedule: min_lr must be in [0, base_lr], got %g (base_lr %g)",
                 (double)s->min_lr, (double)s->base_lr);
    return 0;
}

}
