// The host half of the weight EMA (ema.h, docs/ema.md): CPU twins that run the shared inline functions element by element -- the same
// three roundings per element and the same doubles in the schedule, so the same bits.  No HIP call; host memory only.  Built with
// -ffp-contract=off.
#include "ema.h"

extern "C" int hoig_ema_tick_host(double *state, float *derived, const float *guard) {
    if (!state || !derived) return HOIG_EINVAL;
    if (guard && guard[1] != 0.f) return HOIG_OK;
    ema_tick(state, derived);
    return HOIG_OK;
}

extern "C" int hoig_ema_update_host(float *ema, const float *param, int64_t n, const float *derived, const float *guard) {
    if (!ema_update_ok(ema, param, n, derived)) return HOIG_EINVAL;
    if (guard && guard[1] != 0.f) return HOIG_OK;
    const float w = derived[0];
    for (int64_t i = 0; i < n; ++i) ema[i] = ema_lerp(ema[i], param[i], w);
    return HOIG_OK;
}
