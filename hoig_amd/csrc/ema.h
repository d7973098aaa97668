// EMA of a network's weights (docs/ema.md): the per-element code and the schedule that the kernels of ema.hip and the CPU twins of
// ema_host.cpp share.  Both files are built with -ffp-contract=off, so that `e + (p - e) * w` is three roundings on either side.
#pragma once
#include <stdint.h>

#include "hoig_kernels.h"

#if defined(__HIPCC__)
#define EMA_HD __host__ __device__
#else
#define EMA_HD
#endif

// one element: the average moves towards the parameter by the weight w = (float)(1 - beta)
EMA_HD inline float ema_lerp(float e, float p, float w) { return e + (p - e) * w; }

// The schedule (one thread on the device): state = {decay, warmup (0 or 1), updates}, doubles.  With t updates behind it the decay of
// this one is beta = warmup ? min(decay, (1 + t) / (10 + t)) : decay; derived[0] = (float)(1 - beta), and the count goes to t + 1.
EMA_HD inline void ema_tick(double *state, float *derived) {
    const double decay = state[0], t = state[2];
    double beta = decay;
    if (state[1] != 0.0) {
        const double ramp = (1.0 + t) / (10.0 + t);
        if (ramp < beta) beta = ramp;
    }
    derived[0] = (float)(1.0 - beta);
    state[2] = t + 1.0;
}

// do x[0 .. n) and y[0 .. n) share an element?
inline bool ema_overlap(const float *x, const float *y, int64_t n) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y, len = (uintptr_t)n * sizeof(float);
    return a < b ? b - a < len : a - b < len;
}

inline bool ema_update_ok(const float *ema, const float *param, int64_t n, const float *derived) {
    return ema && param && derived && n > 0 && !(((uintptr_t)ema | (uintptr_t)param) & 15) && !ema_overlap(ema, param, n);
}
