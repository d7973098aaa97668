// Forward-only kernels of the evaluation metrics (hoig_amd/metrics): pooling, image staging, padding, global average, the LPIPS
// layer distance and the fused SSIM level.  NHWC fp32 activations; every reduction is deterministic (partials per workgroup in a
// caller workspace, summed in a fixed order by the last workgroup of an image to arrive, no float atomics).
#include "common.h"

#include <math.h>
#include <type_traits>

namespace {

constexpr int NT = 256;
#define ST ((hipStream_t)stream)

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------- pooling
// F.max_pool2d / F.avg_pool2d (floor output size).  Max pooling pads with -inf; average pooling divides by k*k (count_include_pad:
// the window never passes the padded border with a floor output size) or by the in-image elements of the window.
template <int V>
__global__ __launch_bounds__(NT) void pool2d_kernel(const float *__restrict__ x, float *__restrict__ y, int B, int H, int W, int C,
                                                    int Ho, int Wo, int k, int s, int ph, int pw, int mode, int cip) {
    typedef typename std::conditional<V == 4, float4, float>::type vec;
    const int Cv = C / V;
    const int64_t n = (int64_t)B * Ho * Wo * Cv;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const int cv = (int)(i % Cv);
        int64_t p = i / Cv;
        const int ow = (int)(p % Wo);
        p /= Wo;
        const int oh = (int)(p % Ho);
        const int b = (int)(p / Ho);
        const int h0 = oh * s - ph, w0 = ow * s - pw;
        const int hs = max(h0, 0), ws = max(w0, 0), he = min(h0 + k, H), we = min(w0 + k, W);
        const vec *xb = reinterpret_cast<const vec *>(x + (int64_t)b * H * W * C) + cv;
        float a[V];
        for (int j = 0; j < V; ++j) a[j] = mode == HOIG_POOL_MAX ? -INFINITY : 0.f;
        for (int h = hs; h < he; ++h)
            for (int w = ws; w < we; ++w) {
                const vec v = xb[((int64_t)h * W + w) * Cv];
                const float *e = reinterpret_cast<const float *>(&v);
                for (int j = 0; j < V; ++j) {
                    if (mode == HOIG_POOL_MAX)
                        a[j] = (e[j] > a[j] || isnan(e[j])) ? e[j] : a[j];
                    else
                        a[j] += e[j];
                }
            }
        if (mode == HOIG_POOL_AVG) {
            const float div = (float)(cip ? k * k : (he - hs) * (we - ws));
            for (int j = 0; j < V; ++j) a[j] /= div;
        }
        vec o;
        for (int j = 0; j < V; ++j) reinterpret_cast<float *>(&o)[j] = a[j];
        reinterpret_cast<vec *>(y)[i] = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------- image staging
struct StageAffine {
    float sub[2][4], div[2][4];
    int n;
};

// uint8 HWC -> fp32 NHWC: v = u8 / 255 (ToTensor); optional bilinear resize, align_corners=False (PyTorch's source index
// scale * (dst + 0.5) - 0.5, negative clamped to 0, scale = in / out); then up to two per-channel steps v = (v - sub) / div.
__global__ __launch_bounds__(NT) void stage_u8_kernel(const uint8_t *__restrict__ src, float *__restrict__ y, int B, int Hi, int Wi,
                                                      int C, int Ho, int Wo, int resize, StageAffine a) {
    const int64_t n = (int64_t)B * Ho * Wo;
    const float sh = (float)Hi / (float)Ho, sw = (float)Wi / (float)Wo;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const int ow = (int)(i % Wo);
        const int oh = (int)((i / Wo) % Ho);
        const int b = (int)(i / ((int64_t)Wo * Ho));
        const uint8_t *sb = src + (int64_t)b * Hi * Wi * C;
        int h1 = oh, w1 = ow, h1p = 0, w1p = 0;
        float hl1 = 0.f, wl1 = 0.f;
        if (resize) {
            float rh = sh * ((float)oh + 0.5f) - 0.5f, rw = sw * ((float)ow + 0.5f) - 0.5f;
            rh = rh < 0.f ? 0.f : rh;
            rw = rw < 0.f ? 0.f : rw;
            h1 = min((int)rh, Hi - 1);
            w1 = min((int)rw, Wi - 1);
            h1p = h1 < Hi - 1 ? 1 : 0;
            w1p = w1 < Wi - 1 ? 1 : 0;
            hl1 = rh - (float)h1;
            wl1 = rw - (float)w1;
        }
        const float hl0 = 1.f - hl1, wl0 = 1.f - wl1;
        for (int c = 0; c < C; ++c) {
            float v;
            if (resize) {
                const float v00 = (float)sb[((int64_t)h1 * Wi + w1) * C + c] / 255.f;
                const float v01 = (float)sb[((int64_t)h1 * Wi + w1 + w1p) * C + c] / 255.f;
                const float v10 = (float)sb[((int64_t)(h1 + h1p) * Wi + w1) * C + c] / 255.f;
                const float v11 = (float)sb[((int64_t)(h1 + h1p) * Wi + w1 + w1p) * C + c] / 255.f;
                v = hl0 * (wl0 * v00 + wl1 * v01) + hl1 * (wl0 * v10 + wl1 * v11);
            } else {
                v = (float)sb[((int64_t)oh * Wi + ow) * C + c] / 255.f;
            }
            for (int s = 0; s < a.n; ++s) v = (v - a.sub[s][c]) / a.div[s][c];
            y[i * C + c] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- zero padding
__global__ __launch_bounds__(NT) void pad2d_kernel(const float4 *__restrict__ x, float4 *__restrict__ y, int B, int H, int W, int C4,
                                                   int ph, int pw) {
    const int Hp = H + 2 * ph, Wp = W + 2 * pw;
    const int64_t n = (int64_t)B * Hp * Wp * C4;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const int c = (int)(i % C4);
        int64_t p = i / C4;
        const int w = (int)(p % Wp) - pw;
        p /= Wp;
        const int h = (int)(p % Hp) - ph;
        const int b = (int)(p / Hp);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (h >= 0 && h < H && w >= 0 && w < W) v = x[(((int64_t)b * H + h) * W + w) * C4 + c];
        y[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- global average
// workgroup = 64 channels x 4 pixel phases of one image; the four phase sums are added in a fixed order
__global__ __launch_bounds__(NT) void global_avgpool_kernel(const float *__restrict__ x, float *__restrict__ y, int HW, int C) {
    __shared__ float red[4][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float s = 0.f;
    if (c < C)
        for (int p = r; p < HW; p += 4) s += x[((int64_t)b * HW + p) * C + c];
    red[r][lane] = s;
    __syncthreads();
    if (r == 0 && c < C) y[(int64_t)b * C + c] = ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) / (float)HW;
}

// ---------------------------------------------------------------------------------------------------------------- cross-workgroup finish
// Every workgroup of image b has stored its partials; the last one to arrive returns true (on thread 0 only) and may then read all
// of them.  Agent-scope release before the ticket, acquire after it: correct wherever the workgroups of one image run.
__device__ bool last_arrival(unsigned *cnt, unsigned expected) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x != 0) return false;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t != expected - 1) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return true;
}

// sum of one float per thread over the workgroup (256 threads), fixed order; valid on thread 0
__device__ float block_sum(float v, float *red /*[4]*/) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------------------------------------------- LPIPS layer
constexpr int LP_PIX = 256;   // pixels per workgroup
constexpr int LP_MAXQ = 8;    // channel quads per lane: C <= 16 lanes * 8 * 4 = 512

// 16 lanes per pixel, each holding channel quads l, l + 16, ...: both channel norms, then sum_c w_c (x_c rx - y_c ry)^2
__global__ __launch_bounds__(NT) void lpips_layer_kernel(const float *__restrict__ fx, const float *__restrict__ fy,
                                                         const float *__restrict__ w, float *__restrict__ out, int HW, int C,
                                                         int tiles, float *part, unsigned *cnt) {
    // no fma contraction here: the compiler may fuse the x and y halves differently, and equal maps must give exactly 0
#pragma clang fp contract(off)
    __shared__ float red[16];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int C4 = C >> 2;
    const float4 *w4 = reinterpret_cast<const float4 *>(w);
    const int pend = min((tile + 1) * LP_PIX, HW);
    float acc = 0.f;
    for (int p = tile * LP_PIX + g; p < pend; p += 16) {
        const float4 *px = reinterpret_cast<const float4 *>(fx + ((int64_t)b * HW + p) * C);
        const float4 *py = reinterpret_cast<const float4 *>(fy + ((int64_t)b * HW + p) * C);
        float4 xv[LP_MAXQ], yv[LP_MAXQ];
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int q = 0; q < LP_MAXQ; ++q) {
            const int cq = l + 16 * q;
            if (cq < C4) {
                xv[q] = px[cq];
                yv[q] = py[cq];
                sx += xv[q].x * xv[q].x + xv[q].y * xv[q].y + xv[q].z * xv[q].z + xv[q].w * xv[q].w;
                sy += yv[q].x * yv[q].x + yv[q].y * yv[q].y + yv[q].z * yv[q].z + yv[q].w * yv[q].w;
            }
        }
        for (int o = 8; o > 0; o >>= 1) {
            sx += __shfl_xor(sx, o, 16);
            sy += __shfl_xor(sy, o, 16);
        }
        const float rx = rsqrtf(sx + 1e-10f), ry = rsqrtf(sy + 1e-10f);
        float d = 0.f;
#pragma unroll
        for (int q = 0; q < LP_MAXQ; ++q) {
            const int cq = l + 16 * q;
            if (cq < C4) {
                const float4 wv = w4[cq];
                const float dx = xv[q].x * rx - yv[q].x * ry, dy = xv[q].y * rx - yv[q].y * ry;
                const float dz = xv[q].z * rx - yv[q].z * ry, dw = xv[q].w * rx - yv[q].w * ry;
                d += wv.x * dx * dx + wv.y * dy * dy + wv.z * dz * dz + wv.w * dw * dw;
            }
        }
        for (int o = 8; o > 0; o >>= 1) d += __shfl_xor(d, o, 16);
        acc += d;
    }
    if (l == 0) red[g] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < 16; ++i) s += red[i];
        part[(int64_t)b * tiles + tile] = s;
    }
    if (last_arrival(&cnt[b], (unsigned)tiles)) {
        double tot = 0.0;
        for (int i = 0; i < tiles; ++i) tot += part[(int64_t)b * tiles + i];
        out[b] += (float)(tot / HW);
        cnt[b] = 0;   // (the workspace is left zero-filled for the next call)
    }
}

// ---------------------------------------------------------------------------------------------------------------- SSIM level
constexpr int SS_TW = 64, SS_TH = 16, SS_MAXWIN = 15;
constexpr int SS_IW = SS_TW + SS_MAXWIN - 1, SS_IH = SS_TH + SS_MAXWIN - 1;

struct SsimArgs {
    float g[SS_MAXWIN];
    float C1, C2;
    int win;
};

// One workgroup = a 64 x 16 tile of the valid output of one image, every channel in turn: the x / y tile with its halo in LDS, the
// five moments filtered along W into LDS, then along H, the ssim and cs maps, and the tile's sum of each.  part: [B][C][tiles][2].
__global__ __launch_bounds__(NT) void ssim_kernel(const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ ssim_out,
                                                  float *__restrict__ cs_out, int H, int W, int C, int Ho, int Wo, SsimArgs a,
                                                  int tiles_x, int tiles, float *part, unsigned *cnt) {
    __shared__ float sx[SS_IH][SS_IW], sy[SS_IH][SS_IW];
    __shared__ float hm[5][SS_IH][SS_TW];
    __shared__ float red[4];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int ox0 = (tile % tiles_x) * SS_TW, oy0 = (tile / tiles_x) * SS_TH;
    const int win = a.win, ih = SS_TH + win - 1, iw = SS_TW + win - 1;
    const float *xb = x + (int64_t)b * H * W * C, *yb = y + (int64_t)b * H * W * C;
    for (int c = 0; c < C; ++c) {
        for (int i = threadIdx.x; i < ih * iw; i += NT) {
            const int r = i / iw, q = i % iw, gy = oy0 + r, gx = ox0 + q;
            const bool in = gy < H && gx < W;
            sx[r][q] = in ? xb[((int64_t)gy * W + gx) * C + c] : 0.f;
            sy[r][q] = in ? yb[((int64_t)gy * W + gx) * C + c] : 0.f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < ih * SS_TW; i += NT) {
            const int r = i / SS_TW, q = i % SS_TW;
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
            for (int t = 0; t < win; ++t) {
                const float u = sx[r][q + t], v = sy[r][q + t], gt = a.g[t];
                m0 += gt * u;
                m1 += gt * v;
                m2 += gt * (u * u);
                m3 += gt * (v * v);
                m4 += gt * (u * v);
            }
            hm[0][r][q] = m0; hm[1][r][q] = m1; hm[2][r][q] = m2; hm[3][r][q] = m3; hm[4][r][q] = m4;
        }
        __syncthreads();
        float ts = 0.f, tc = 0.f;
        for (int i = threadIdx.x; i < SS_TH * SS_TW; i += NT) {
            const int r = i / SS_TW, q = i % SS_TW;
            if (oy0 + r >= Ho || ox0 + q >= Wo) continue;
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
            for (int t = 0; t < win; ++t) {
                const float gt = a.g[t];
                m0 += gt * hm[0][r + t][q];
                m1 += gt * hm[1][r + t][q];
                m2 += gt * hm[2][r + t][q];
                m3 += gt * hm[3][r + t][q];
                m4 += gt * hm[4][r + t][q];
            }
            const float mu11 = m0 * m0, mu22 = m1 * m1, mu12 = m0 * m1;
            const float s11 = m2 - mu11, s22 = m3 - mu22, s12 = m4 - mu12;
            const float cs = (2.f * s12 + a.C2) / (s11 + s22 + a.C2);
            tc += cs;
            ts += ((2.f * mu12 + a.C1) / (mu11 + mu22 + a.C1)) * cs;
        }
        ts = block_sum(ts, red);
        tc = block_sum(tc, red);
        if (threadIdx.x == 0) {
            float *pp = part + (((int64_t)b * C + c) * tiles + tile) * 2;
            pp[0] = ts;
            pp[1] = tc;
        }
        __syncthreads();   // (LDS is refilled for the next channel)
    }
    if (last_arrival(&cnt[b], (unsigned)tiles)) {
        const double inv = 1.0 / ((double)Ho * Wo);
        for (int c = 0; c < C; ++c) {
            const float *pp = part + ((int64_t)b * C + c) * tiles * 2;
            double s0 = 0.0, s1 = 0.0;
            for (int i = 0; i < tiles; ++i) {
                s0 += pp[2 * i];
                s1 += pp[2 * i + 1];
            }
            ssim_out[(int64_t)b * C + c] = (float)(s0 * inv);
            cs_out[(int64_t)b * C + c] = (float)(s1 * inv);
        }
        cnt[b] = 0;
    }
}

int ssim_tiles(int H, int W, int win, int *tiles_x) {
    const int Ho = H - win + 1, Wo = W - win + 1;
    *tiles_x = (int)hoig_cdiv(Wo, SS_TW);
    return *tiles_x * (int)hoig_cdiv(Ho, SS_TH);
}

inline int64_t align256(int64_t n) { return (n + 255) & ~(int64_t)255; }

}  // namespace

extern "C" int hoig_pool2d_fwd(const float *x, float *y, int B, int H, int W, int C, int k, int stride, int pad_h, int pad_w, int mode,
                               int count_include_pad, hoig_stream_t stream) {
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0 || stride <= 0) return HOIG_EINVAL;
    if (mode != HOIG_POOL_MAX && mode != HOIG_POOL_AVG) return HOIG_EINVAL;
    if (pad_h < 0 || pad_w < 0 || 2 * pad_h > k || 2 * pad_w > k) return HOIG_EINVAL;   // (F.*_pool2d: pad <= k / 2)
    const int Ho = (H + 2 * pad_h - k) / stride + 1, Wo = (W + 2 * pad_w - k) / stride + 1;
    if (H + 2 * pad_h < k || W + 2 * pad_w < k) return HOIG_EINVAL;
    if (C % 4 == 0 && aligned16(x) && aligned16(y))
        pool2d_kernel<4><<<hoig_stream_grid((int64_t)B * Ho * Wo * C / 4, NT), NT, 0, ST>>>(x, y, B, H, W, C, Ho, Wo, k, stride, pad_h,
                                                                                             pad_w, mode, count_include_pad);
    else
        pool2d_kernel<1><<<hoig_stream_grid((int64_t)B * Ho * Wo * C, NT), NT, 0, ST>>>(x, y, B, H, W, C, Ho, Wo, k, stride, pad_h,
                                                                                         pad_w, mode, count_include_pad);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_stage_images_u8(const uint8_t *src, float *y, int B, int Hi, int Wi, int C, int Ho, int Wo, int n_affine,
                                    const float *affine, hoig_stream_t stream) {
    if (!src || !y || B <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || C > 4) return HOIG_EINVAL;
    if (n_affine < 0 || n_affine > 2 || (n_affine > 0 && !affine)) return HOIG_EINVAL;
    StageAffine a = {};
    a.n = n_affine;
    for (int s = 0; s < n_affine; ++s)
        for (int c = 0; c < C; ++c) {
            a.sub[s][c] = affine[(2 * s) * C + c];
            a.div[s][c] = affine[(2 * s + 1) * C + c];
        }
    const int resize = (Ho != Hi || Wo != Wi) ? 1 : 0;
    stage_u8_kernel<<<hoig_stream_grid((int64_t)B * Ho * Wo, NT), NT, 0, ST>>>(src, y, B, Hi, Wi, C, Ho, Wo, resize, a);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_pad2d(const float *x, float *y, int B, int H, int W, int C, int pad_h, int pad_w, hoig_stream_t stream) {
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || pad_h < 0 || pad_w < 0) return HOIG_EINVAL;
    if (C % 4 || !aligned16(x) || !aligned16(y)) return HOIG_EUNSUPPORTED;
    const int64_t n = (int64_t)B * (H + 2 * pad_h) * (W + 2 * pad_w) * (C / 4);
    pad2d_kernel<<<hoig_stream_grid(n, NT), NT, 0, ST>>>(reinterpret_cast<const float4 *>(x), reinterpret_cast<float4 *>(y), B, H, W,
                                                         C / 4, pad_h, pad_w);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int hoig_global_avgpool(const float *x, float *y, int B, int HW, int C, hoig_stream_t stream) {
    if (!x || !y || B <= 0 || HW <= 0 || C <= 0 || B > 65535) return HOIG_EINVAL;
    global_avgpool_kernel<<<dim3((unsigned)hoig_cdiv(C, 64), B), NT, 0, ST>>>(x, y, HW, C);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int64_t hoig_lpips_workspace_bytes(int B, int HW) {
    if (B <= 0 || HW <= 0) return -1;
    return align256((int64_t)B * 4) + (int64_t)B * hoig_cdiv(HW, LP_PIX) * 4;
}

extern "C" int hoig_lpips_layer(const float *fx, const float *fy, const float *w, float *out, int B, int HW, int C, void *workspace,
                                hoig_stream_t stream) {
    if (!fx || !fy || !w || !out || !workspace || B <= 0 || HW <= 0 || C <= 0 || B > 65535) return HOIG_EINVAL;
    if (C % 4 || C > 16 * 4 * LP_MAXQ || !aligned16(fx) || !aligned16(fy) || !aligned16(w)) return HOIG_EUNSUPPORTED;
    const int tiles = (int)hoig_cdiv(HW, LP_PIX);
    unsigned *cnt = (unsigned *)workspace;   // (first: the same words for every layer's launch on one workspace)
    float *part = (float *)((char *)workspace + align256((int64_t)B * 4));
    lpips_layer_kernel<<<dim3(tiles, B), NT, 0, ST>>>(fx, fy, w, out, HW, C, tiles, part, cnt);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

extern "C" int64_t hoig_ssim_workspace_bytes(int B, int H, int W, int C, int win) {
    if (B <= 0 || C <= 0 || win <= 0 || H < win || W < win) return -1;
    int tx;
    const int tiles = ssim_tiles(H, W, win, &tx);
    return align256((int64_t)B * 4) + (int64_t)B * C * tiles * 2 * 4;
}

extern "C" int hoig_ssim(const float *x, const float *y, float *ssim_out, float *cs_out, int B, int H, int W, int C, float data_range,
                         float K1, float K2, int win, float sigma, void *workspace, hoig_stream_t stream) {
    if (!x || !y || !ssim_out || !cs_out || !workspace || B <= 0 || C <= 0 || B > 65535 || !(sigma > 0.f)) return HOIG_EINVAL;
    if (win <= 0 || !(win & 1) || H < win || W < win) return HOIG_EINVAL;
    if (win > SS_MAXWIN) return HOIG_EUNSUPPORTED;
    SsimArgs a = {};
    a.win = win;
    // pytorch_msssim's window: exp(-(t - win / 2)^2 / (2 sigma^2)) over t = 0 .. win-1, normalised to sum 1
    double g[SS_MAXWIN], gs = 0.0;
    for (int t = 0; t < win; ++t) {
        const double u = t - win / 2;
        g[t] = exp(-(u * u) / (2.0 * (double)sigma * sigma));
        gs += g[t];
    }
    for (int t = 0; t < win; ++t) a.g[t] = (float)(g[t] / gs);
    a.C1 = (float)(((double)K1 * data_range) * ((double)K1 * data_range));
    a.C2 = (float)(((double)K2 * data_range) * ((double)K2 * data_range));
    int tiles_x;
    const int tiles = ssim_tiles(H, W, win, &tiles_x);
    unsigned *cnt = (unsigned *)workspace;
    float *part = (float *)((char *)workspace + align256((int64_t)B * 4));
    ssim_kernel<<<dim3(tiles, B), NT, 0, ST>>>(x, y, ssim_out, cs_out, H, W, C, H - win + 1, W - win + 1, a, tiles_x, tiles, part, cnt);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}
