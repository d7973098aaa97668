// The host half of the opt-in GAN objectives (gan_loss.h, docs/gan_objectives.md): CPU twins that run the shared inline functions in
// the order the kernels run them -- the same fp32 roundings per element, the same doubles in the same order through the threads, the
// workgroup's tree and the partials, the same tick -- so, outside the logistic objective (whose expf / log1pf are the host library's
// here), the same bits.  No HIP call; host memory only.  Built with -ffp-contract=off.
#include "gan_loss.h"

namespace {

void run(const gan_args &p, const gan_finish_args &f) {
    double partials[GAN_MAX_GRID * GAN_SUMS];
    gan_acc acc[GAN_NT];
    for (int g = 0; g < f.grid; ++g) {
        for (int t = 0; t < GAN_NT; ++t) acc[t] = gan_thread(p, f.grid, g, t);
        const gan_acc w = gan_tree(acc);
        for (int j = 0; j < GAN_SUMS; ++j) partials[g * GAN_SUMS + j] = w.s[j];
    }
    gan_finish(f, partials);
}

}  // namespace

extern "C" int hoig_gan_d_loss_host(int mode, const float *a, int64_t n_a, const float *b, int64_t n_b, double s, double lambda_lc,
                                    int lecam_form, uint64_t *state, float *da, float *db, float *term, float *mean_a, float *mean_b,
                                    float *reg) {
    gan_args p;
    gan_finish_args f;
    if (!gan_d_pack(mode, a, n_a, b, n_b, s, lambda_lc, lecam_form, state, da, db, term, mean_a, mean_b, reg, &p, &f)) return HOIG_EINVAL;
    run(p, f);
    return HOIG_OK;
}

extern "C" int hoig_gan_g_loss_host(int mode, const float *b, int64_t n_b, double s, float *db, float *term) {
    gan_args p;
    gan_finish_args f;
    if (!gan_g_pack(mode, b, n_b, s, db, term, &p, &f)) return HOIG_EINVAL;
    run(p, f);
    return HOIG_OK;
}
