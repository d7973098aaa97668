// hoig_set_tuning: the one table of kernel-variant choices (see include/hoig_kernels.h).
#include <cstring>
#include "hoig_kernels.h"
#include "tuning.h"
#include "conv_route.h"

namespace {
struct Entry {
    const char *key;
    int value;
};
Entry g_table[HOIG_TUNE_COUNT] = {
    {"igemm16", 1},
    {"s2_16", 1},
    {"flat5", 2},
    {"wflat5", 1},
    {"head16", 1},
    {"d_early", 1},
    {"split_grads", 1},
    {"pair", 2},
    {"wdma16", 2},
    {"s2_pipe", 1},
    {"norm_in", 1},
    {"wino8", 0},
    // the attention's WIDE valid 5x5 layers (72 / 68 / 136 / 132 pixels, which the flattened-axis kernel declines) on the 2-D-tiled
    // halo kernel of conv_halo5.hip, forward and data gradient; 0: the generic implicit GEMM, as before that kernel existed;
    // 2: as 1, without its split over K on launches of few tiles
    {"halo5", 1},
    // the PNG decoder's inflate window (png_decode.hip): 0 a 32 KiB ring in LDS; 1 the image's own filtered stream in the workspace, a
    // workgroup-scope fence between a store and a later read of it (the A/B of profiles/png_decode.txt)
    {"png_window", 0},
};
}  // namespace

int hoig_tuning(int id) { return (id >= 0 && id < HOIG_TUNE_COUNT) ? g_table[id].value : 0; }

extern "C" int hoig_set_tuning(const char *key, int value) {
    if (!key) return -1;
    for (int i = 0; i < HOIG_TUNE_COUNT; ++i)
        if (strcmp(g_table[i].key, key) == 0) {
            const int prev = g_table[i].value;
            if (value >= 0) g_table[i].value = value;
            return prev;
        }
    return -1;
}

// the route record (conv_route.h): the launcher that ran last on this thread, per pass
thread_local int hoig_route_last[3] = {0, 0, 0};

extern "C" int hoig_conv_last_route(int which) { return (which >= 0 && which < 3) ? hoig_route_last[which] : -1; }

extern "C" const char *hoig_conv_route_name(int id) {
    static const char *const names[HOIG_ROUTE_COUNT] = {
        "none",
#define HOIG_R_W(n) #n,
#define HOIG_R_D(n) "dgrad_" #n,
#define HOIG_R_F(n) "fwd_" #n,
#define HOIG_R_FD(n) "fwd_" #n, "dgrad_" #n,
        HOIG_CONV_ROUTES(HOIG_R_W, HOIG_R_D, HOIG_R_F, HOIG_R_FD)
#undef HOIG_R_W
#undef HOIG_R_D
#undef HOIG_R_F
#undef HOIG_R_FD
    };
    return (id >= 0 && id < HOIG_ROUTE_COUNT) ? names[id] : nullptr;
}
