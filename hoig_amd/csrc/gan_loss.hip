// The opt-in GAN objectives on the device (docs/gan_objectives.md; the per-element code, the state, the tick and the layout of the
// sums: gan_loss.h).  A head is two launches on the caller's stream: gan_partials_kernel reads every logit once, writes the
// gradients and one partial of six doubles per workgroup; gan_finish_kernel, one thread, adds the partials first to last, adds the
// results to the fp32 slots and ticks the LeCam state.  The second launch runs behind the first in stream order, so every workgroup
// of the first has read the anchors as they stood before the tick.  Nothing here synchronises, allocates, waits for another
// workgroup or uses a floating-point atomic.  The work is a few tens of kilobytes: the kernels are launch-bound and are not tuned for
// bandwidth.  Built with -ffp-contract=off.
#include "common.h"
#include "gan_loss.h"

namespace {

__global__ __launch_bounds__(GAN_NT) void gan_partials_kernel(gan_args p, double *__restrict__ partials) {
    __shared__ gan_acc sh[GAN_NT];
    const int t = threadIdx.x;
    sh[t] = gan_thread(p, (int)gridDim.x, (int)blockIdx.x, t);
    __syncthreads();
    if (t >= 64) return;                                    // (wave 0 goes on alone: no barrier below)
    // the halving tree's steps 128 and 64 ...
    gan_acc a = gan_join(gan_join(sh[t], sh[t + 128]), gan_join(sh[t + 64], sh[t + 192]));
    // ... and its steps 32 .. 1: lane t < o holds acc[t] + acc[t + o], as the tree does (the other lanes' sums are not used)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        gan_acc b;
#pragma unroll
        for (int j = 0; j < GAN_SUMS; ++j) b.s[j] = __shfl_xor(a.s[j], o, 64);
        a = gan_join(a, b);
    }
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < GAN_SUMS; ++j) partials[(int64_t)blockIdx.x * GAN_SUMS + j] = a.s[j];
    }
}

__global__ void gan_finish_kernel(gan_finish_args f, const double *__restrict__ partials) {
    if (threadIdx.x == 0 && blockIdx.x == 0) gan_finish(f, partials);
}

int launch(const gan_args &p, const gan_finish_args &f, void *workspace, int64_t workspace_bytes, hoig_stream_t stream) {
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < gan_workspace_bytes(p.n_a, p.n_b)) return HOIG_EINVAL;
    double *partials = static_cast<double *>(workspace);
    const int rc = hoig_launch<gan_partials_kernel>(dim3((unsigned)f.grid), dim3(GAN_NT), 0, (hipStream_t)stream, p, partials);
    if (rc != HOIG_OK) return rc;
    return hoig_launch<gan_finish_kernel>(dim3(1), dim3(64), 0, (hipStream_t)stream, f, (const double *)partials);
}

}  // namespace

extern "C" int64_t hoig_gan_d_loss_workspace_bytes(int64_t n_a, int64_t n_b) { return n_a <= 0 ? -1 : gan_workspace_bytes(n_a, n_b); }
extern "C" int64_t hoig_gan_g_loss_workspace_bytes(int64_t n_b) { return gan_workspace_bytes(0, n_b); }

extern "C" int hoig_gan_d_loss(int mode, const float *a, int64_t n_a, const float *b, int64_t n_b, double s, double lambda_lc,
                               int lecam_form, uint64_t *state, float *da, float *db, float *term, float *mean_a, float *mean_b,
                               float *reg, void *workspace, int64_t workspace_bytes, hoig_stream_t stream) {
    gan_args p;
    gan_finish_args f;
    if (!gan_d_pack(mode, a, n_a, b, n_b, s, lambda_lc, lecam_form, state, da, db, term, mean_a, mean_b, reg, &p, &f)) return HOIG_EINVAL;
    return launch(p, f, workspace, workspace_bytes, stream);
}

extern "C" int hoig_gan_g_loss(int mode, const float *b, int64_t n_b, double s, float *db, float *term, void *workspace,
                               int64_t workspace_bytes, hoig_stream_t stream) {
    gan_args p;
    gan_finish_args f;
    if (!gan_g_pack(mode, b, n_b, s, db, term, &p, &f)) return HOIG_EINVAL;
    return launch(p, f, workspace, workspace_bytes, stream);
}
