// JPEG frames decoded on the device (the loader's rgb/*.jpg and color_%06d.jpg; include/hoig_kernels.h has the interface, DESIGN.md
// section 10 the rules).  Three kernels per batch (five launches with the parallel entropy stage):
//
//   jpeg_entropy_kernel   Huffman decode.  Serial inside a restart interval by nature (a code's position depends on every code before
//                         it), so one workgroup of ONE wave takes an (image, interval) pair: lanes 0-5 build the image's lookup tables in
//                         LDS from the canonical form, then lane 0 runs jpeg_entropy.h's block loop -- the code hoig_jpeg_entropy_host
//                         runs on the CPU -- while the whole wave feeds it: the stream comes through a 4 KB LDS window that all 64 lanes
//                         refill with 16-byte loads (a byte at a time from global memory would cost a round trip per byte), and each
//                         finished block leaves as one 128-byte row, zeros included, so the coefficient buffer needs no clearing.
//   jpeg_entropy_par_kernel  (hoig_jpeg_decode_bgr_u8_par, instead of the kernel above) Huffman decode that is parallel INSIDE an interval:
//                         jpeg_parallel.h's self-synchronising sub-sequences.  One workgroup of 128 / 256 / 512 threads (sub-sequences
//                         of 256 / 128 / 32-64 bytes) takes an (image, interval) pair and walks it in chunks of at most 32 KB, which all
//                         threads stage in LDS with 16-byte loads (a dword of padding behind every sub-sequence keeps neighbouring
//                         lanes in different banks); the lanes' states, block counts and DC sums live in LDS; rounds are separated by
//                         workgroup barriers with an "anything changed" vote, and only lanes whose state changed decode again.  The
//                         coefficients are zeroed by one memset in front of it (a lane that starts inside a block continues it).
//   jpeg_entropy_flagged_kernel  the serial kernel again, for the intervals the parallel one found irregular (corrupt streams): it
//                         writes their blocks and the status word; every other workgroup ends at once.
//   jpeg_idct_kernel      dequantise + jidctint's islow IDCT, one thread per 8 x 8 block, into padded uint8 component planes.
//   jpeg_colour_kernel    libjpeg's fancy upsampling (h2v1 / h2v2 triangle filters) and fixed-point YCbCr -> RGB, one thread per pixel,
//                         written as interleaved BGR.
//
// All integer arithmetic; the result equals Pillow (libjpeg-turbo) byte for byte on encoder-made files.  A corrupt stream sets its
// image's status word and stops; nothing is read or written outside the buffers the plans describe (the entry points check the plans).
#include "common.h"
#include "jpeg_entropy.h"
#include "jpeg_parallel.h"

namespace {

constexpr int WIN = 4096;   // LDS window on the stream, bytes

struct DevCtx {
    const uint8_t *bytes;   // the packed buffer
    int64_t nbytes, data_off;
    uint8_t *win;
    int16_t *blk;
    int base;               // the window holds scan positions [base, base + WIN)
    int lane, natural;      // natural: where this lane's zigzag position lies in the block

    __device__ uint8_t byte(int pos) const { return win[pos - base]; }
    __device__ void window(int pos) {
        if (pos >= base && pos + JPEG_BLOCK_MAX_BYTES + 16 <= base + WIN) return;
        __syncthreads();
        const int64_t abs0 = (data_off + pos) & ~(int64_t)15;
        base = (int)(abs0 - data_off);
#pragma unroll
        for (int k = 0; k < WIN / 16 / 64; ++k) {
            const int slot = k * 64 + lane;
            const int64_t a = abs0 + (int64_t)slot * 16;
            if (a + 16 <= nbytes) reinterpret_cast<uint4 *>(win)[slot] = *reinterpret_cast<const uint4 *>(bytes + a);
        }
        __syncthreads();
    }
    __device__ int16_t *stage() {
        blk[lane] = 0;
        __syncthreads();
        return blk;
    }
    __device__ bool decoder() const { return lane == 0; }
    __device__ int share(int v) const { return __shfl(v, 0, 64); }
    __device__ void flush(int16_t *dst) {
        __syncthreads();
        dst[natural] = blk[lane];
        __syncthreads();
    }
};

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t *__restrict__ bytes, int64_t nbytes,
                                                          const hoig_jpeg_plan *__restrict__ plans,
                                                          const int32_t *__restrict__ intervals, int32_t *__restrict__ status,
                                                          char *__restrict__ workspace) {
    const int img = blockIdx.y, iv = blockIdx.x, lane = threadIdx.x;
    const hoig_jpeg_plan &P = plans[img];
    if (iv >= P.n_intervals) return;
    __shared__ JpegHuff tab[6];                      // DC of components 0-2, then AC
    __shared__ __attribute__((aligned(16))) uint8_t win[WIN];
    __shared__ int16_t blk[64];
    bool ok = true;
    if (lane < 6 && lane % 3 < P.ncomp) {
        const int c = lane % 3;
        ok = lane < 3 ? jpeg_build_huff(P.dc_counts[c], P.dc_vals[c], 16, &tab[lane]) : jpeg_build_huff(P.ac_counts[c], P.ac_vals[c], 256, &tab[lane]);
    }
    __syncthreads();
    if (__any(!ok)) {
        if (lane == 0) atomicOr(status + img, (int32_t)HOIG_JPEG_ECODE);
        return;
    }
    DevCtx cx;
    cx.bytes = bytes; cx.nbytes = nbytes; cx.data_off = P.data_off;
    cx.win = win; cx.blk = blk; cx.base = -(1 << 30); cx.lane = lane; cx.natural = jpeg_natural(lane);
    const int err = jpeg_decode_interval(P, tab, tab + 3, intervals + P.interval_first, iv,
                                         reinterpret_cast<int16_t *>(workspace + P.coef_off), cx);
    if (err && lane == 0) atomicOr(status + img, (int32_t)err);
}

// ---- the entropy stage, parallel inside an interval (jpeg_parallel.h)
constexpr int PAR_CHUNK = 32768;                            // bytes of a chunk in LDS
constexpr int PAR_W_MAX = 512;                              // threads of a workgroup = lanes of a chunk = min(PAR_W_MAX, PAR_CHUNK / S)
constexpr int PAR_WIN = PAR_CHUNK + JPEG_PAR_OVER + 32;     // staged bytes: the chunk, what a lane reads behind it, 16-byte alignment
constexpr int PAR_LDS = PAR_WIN + PAR_WIN / 32 * 4;         // with a dword of padding behind every S bytes (S >= 32)

template <int W>
struct DevParCtx {
    const uint8_t *bytes;
    int64_t nbytes, data_off;
    uint8_t *win;
    int base, logs, tid;
    JpegParTab T;

    // Lanes read S bytes apart: 32 dwords for S = 128, i.e. all of them in two banks.  A dword of padding behind every S bytes puts
    // neighbouring lanes one bank apart.  (The index is clamped: a position outside the staged range reads the window's last byte.)
    __device__ unsigned at(unsigned rel) const { return rel + ((rel >> logs) << 2); }
    __device__ uint8_t byte(int pos) const { return win[min(at((unsigned)(pos - base)), (unsigned)(PAR_LDS - 1))]; }
    __device__ void stage(int pos0, int pos1) {
        __syncthreads();
        const int64_t abs0 = (data_off + pos0) & ~(int64_t)15;
        base = (int)(abs0 - data_off);
        const int slots = min((int)((data_off + pos1 - abs0 + 15) >> 4), PAR_WIN / 16);
        for (int slot = tid; slot < slots; slot += W) {
            const int64_t a = abs0 + (int64_t)slot * 16;
            if (a + 16 <= nbytes) {
                const uint4 v = *reinterpret_cast<const uint4 *>(bytes + a);
                uint32_t *d = reinterpret_cast<uint32_t *>(win + at((unsigned)slot * 16u));     // (16 bytes never straddle a padding)
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        }
        __syncthreads();
    }
    __device__ int first() const { return tid; }
    __device__ int step() const { return W; }
    __device__ void barrier() const { __syncthreads(); }
    __device__ bool any(bool v) const { return __syncthreads_or(v) != 0; }
    __device__ JpegParTab *tab() { return &T; }
};

// One workgroup per (image, interval): the tables in LDS as above, the chunk's bytes and its lanes' tables in LDS, then
// jpeg_par_interval.  irregular[interval_first + iv] = 1: jpeg_entropy_flagged_kernel decodes this interval again.
template <int W>
__global__ __launch_bounds__(W) void jpeg_entropy_par_kernel(const uint8_t *__restrict__ bytes, int64_t nbytes,
                                                                 const hoig_jpeg_plan *__restrict__ plans,
                                                                 const int32_t *__restrict__ intervals, int S, int logs,
                                                                 int32_t *__restrict__ irregular, char *__restrict__ workspace) {
    const int img = blockIdx.y, iv = blockIdx.x, tid = threadIdx.x;
    const hoig_jpeg_plan &P = plans[img];
    if (iv >= P.n_intervals) return;
    __shared__ JpegHuff tab[6];
    __shared__ __attribute__((aligned(16))) uint8_t win[PAR_LDS];
    __shared__ uint32_t state[W], cand[W];
    __shared__ int32_t dirty[W], nblk[W], dc0[W], dc1[W], dc2[W], carry[8];
    bool ok = true;
    if (tid < 6 && tid % 3 < P.ncomp) {
        const int c = tid % 3;
        ok = tid < 3 ? jpeg_build_huff(P.dc_counts[c], P.dc_vals[c], 16, &tab[tid]) : jpeg_build_huff(P.ac_counts[c], P.ac_vals[c], 256, &tab[tid]);
    }
    int bad = __syncthreads_or(!ok);                 // (a table that is no prefix code: the serial kernel reports it)
    if (!bad) {
        DevParCtx<W> cx;
        cx.bytes = bytes; cx.nbytes = nbytes; cx.data_off = P.data_off;
        cx.win = win; cx.base = 0; cx.logs = logs; cx.tid = tid;
        cx.T.state = state; cx.T.cand = cand; cx.T.dirty = dirty; cx.T.nblk = nblk; cx.T.dc0 = dc0; cx.T.dc1 = dc1; cx.T.dc2 = dc2;
        cx.T.carry = carry;
        bad = jpeg_par_interval(P, tab, tab + 3, intervals + P.interval_first, iv, reinterpret_cast<int16_t *>(workspace + P.coef_off), S,
                                W, cx, nullptr, nullptr);
    }
    if (tid == 0) irregular[P.interval_first + iv] = bad;
}

// jpeg_entropy_kernel for the intervals jpeg_entropy_par_kernel marked; every other workgroup ends at once.  (The body is that
// kernel's, repeated: it is the pinned serial path, and stays untouched.)
__global__ __launch_bounds__(64) void jpeg_entropy_flagged_kernel(const uint8_t *__restrict__ bytes, int64_t nbytes,
                                                                  const hoig_jpeg_plan *__restrict__ plans,
                                                                  const int32_t *__restrict__ intervals,
                                                                  const int32_t *__restrict__ irregular, int32_t *__restrict__ status,
                                                                  char *__restrict__ workspace) {
    const int img = blockIdx.y, iv = blockIdx.x, lane = threadIdx.x;
    const hoig_jpeg_plan &P = plans[img];
    if (iv >= P.n_intervals || !irregular[P.interval_first + iv]) return;
    __shared__ JpegHuff tab[6];
    __shared__ __attribute__((aligned(16))) uint8_t win[WIN];
    __shared__ int16_t blk[64];
    bool ok = true;
    if (lane < 6 && lane % 3 < P.ncomp) {
        const int c = lane % 3;
        ok = lane < 3 ? jpeg_build_huff(P.dc_counts[c], P.dc_vals[c], 16, &tab[lane]) : jpeg_build_huff(P.ac_counts[c], P.ac_vals[c], 256, &tab[lane]);
    }
    __syncthreads();
    if (__any(!ok)) {
        if (lane == 0) atomicOr(status + img, (int32_t)HOIG_JPEG_ECODE);
        return;
    }
    DevCtx cx;
    cx.bytes = bytes; cx.nbytes = nbytes; cx.data_off = P.data_off;
    cx.win = win; cx.blk = blk; cx.base = -(1 << 30); cx.lane = lane; cx.natural = jpeg_natural(lane);
    const int err = jpeg_decode_interval(P, tab, tab + 3, intervals + P.interval_first, iv,
                                         reinterpret_cast<int16_t *>(workspace + P.coef_off), cx);
    if (err && lane == 0) atomicOr(status + img, (int32_t)err);
}

// jidctint.c (islow): CONST_BITS 13, PASS1_BITS 2
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299,
              F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

// eight samples at stride S, in place; the results are descaled by `shift` (with rounding)
template <int S>
__device__ __forceinline__ void idct8(int *d, int shift) {
    int z2 = d[2 * S], z3 = d[6 * S];
    int z1 = (z2 + z3) * F_0_541;
    int tmp2 = z1 + z3 * (-F_1_847), tmp3 = z1 + z2 * F_0_765;
    z2 = d[0];
    z3 = d[4 * S];
    int tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7 * S]; tmp1 = d[5 * S]; tmp2 = d[3 * S]; tmp3 = d[1 * S];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F_1_175;
    tmp0 *= F_0_298; tmp1 *= F_2_053; tmp2 *= F_3_072; tmp3 *= F_1_501;
    z1 *= -F_0_899; z2 *= -F_2_562; z3 *= -F_1_961; z4 *= -F_0_390;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const int r = 1 << (shift - 1);
    d[0] = (tmp10 + tmp3 + r) >> shift; d[7 * S] = (tmp10 - tmp3 + r) >> shift;
    d[1 * S] = (tmp11 + tmp2 + r) >> shift; d[6 * S] = (tmp11 - tmp2 + r) >> shift;
    d[2 * S] = (tmp12 + tmp1 + r) >> shift; d[5 * S] = (tmp12 - tmp1 + r) >> shift;
    d[3 * S] = (tmp13 + tmp0 + r) >> shift; d[4 * S] = (tmp13 - tmp0 + r) >> shift;
}

__device__ __forceinline__ int clamp255(int v) { return min(255, max(0, v)); }

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const hoig_jpeg_plan *__restrict__ plans, char *__restrict__ workspace) {
    const hoig_jpeg_plan &P = plans[blockIdx.y];
    const JpegGeom g = jpeg_geometry(P);
    const int16_t *coef = reinterpret_cast<const int16_t *>(workspace + P.coef_off);
    uint8_t *planes = reinterpret_cast<uint8_t *>(workspace + P.plane_off);
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < g.blocks; t += (int64_t)gridDim.x * 256) {
        const int c = P.ncomp == 3 ? (t >= g.first[2] ? 2 : (t >= g.first[1] ? 1 : 0)) : 0;
        const int64_t local = t - g.first[c];
        const int by = (int)(local / g.bw[c]), bx = (int)(local % g.bw[c]);
        const uint16_t *q = P.quant[c];
        int ws[64];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint4 v = reinterpret_cast<const uint4 *>(coef + t * 64)[k];
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ws[k * 8 + 2 * j] = (int)(int16_t)(w[j] & 0xffffu) * (int)q[k * 8 + 2 * j];
                ws[k * 8 + 2 * j + 1] = (int)(int16_t)(w[j] >> 16) * (int)q[k * 8 + 2 * j + 1];
            }
        }
#pragma unroll
        for (int col = 0; col < 8; ++col) idct8<8>(ws + col, 11);      // columns: CONST_BITS - PASS1_BITS
        const int stride = g.bw[c] * 8;
        uint8_t *dst = planes + g.first[c] * 64 + (int64_t)by * 8 * stride + bx * 8;
#pragma unroll
        for (int row = 0; row < 8; ++row) {
            idct8<1>(ws + row * 8, 18);                                // rows: CONST_BITS + PASS1_BITS + 3
            unsigned lo = 0, hi = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo |= (unsigned)clamp255(ws[row * 8 + j] + 128) << (8 * j);
                hi |= (unsigned)clamp255(ws[row * 8 + 4 + j] + 128) << (8 * j);
            }
            *reinterpret_cast<uint2 *>(dst + (int64_t)row * stride) = make_uint2(lo, hi);
        }
    }
}

// The chroma sample libjpeg's upsampler gives at full-resolution (x, y).  pl: the padded plane, cw x ch: its REAL samples
// (ceil(W / 2) x ceil(H / vs)); a plane of at most two columns is replicated, not filtered (jdsample.c: downsampled_width > 2).
__device__ __forceinline__ int chroma_at(const uint8_t *__restrict__ pl, int stride, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return pl[(int64_t)y * stride + x];
    const int i = x >> 1;
    if (vs == 1) {                                   // h2v1_fancy_upsample
        const uint8_t *row = pl + (int64_t)y * stride;
        const int a = row[i];
        if (cw <= 2) return a;
        if (x & 1) return i == cw - 1 ? a : (3 * a + row[i + 1] + 2) >> 2;
        return i == 0 ? a : (3 * a + row[i - 1] + 1) >> 2;
    }
    const int j = y >> 1;                            // h2v2_fancy_upsample
    if (cw <= 2) return pl[(int64_t)j * stride + i];
    const int jf = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
    const uint8_t *near = pl + (int64_t)j * stride, *far = pl + (int64_t)jf * stride;
    const int cs = 3 * near[i] + far[i];
    if (x & 1) return i == cw - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const hoig_jpeg_plan *__restrict__ plans, const char *__restrict__ workspace,
                                                          uint8_t *__restrict__ out) {
    const hoig_jpeg_plan &P = plans[blockIdx.y];
    const JpegGeom g = jpeg_geometry(P);
    const int W = P.width, H = P.height;
    const uint8_t *planes = reinterpret_cast<const uint8_t *>(workspace + P.plane_off);
    uint8_t *dst = out + P.out_off;
    const int hs = g.h[0], vs = g.v[0];
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    const int64_t n = (int64_t)W * H;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % W), y = (int)(i / W);
        const int Y = planes[(int64_t)y * g.bw[0] * 8 + x];
        int r = Y, gr = Y, b = Y;
        if (P.ncomp == 3) {
            const int cb = chroma_at(planes + g.first[1] * 64, g.bw[1] * 8, cw, ch, hs, vs, x, y) - 128;
            const int cr = chroma_at(planes + g.first[2] * 64, g.bw[2] * 8, cw, ch, hs, vs, x, y) - 128;
            r = clamp255(Y + ((91881 * cr + 32768) >> 16));
            b = clamp255(Y + ((116130 * cb + 32768) >> 16));
            gr = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        }
        dst[i * 3] = (uint8_t)b;
        dst[i * 3 + 1] = (uint8_t)gr;
        dst[i * 3 + 2] = (uint8_t)r;
    }
}

struct BatchDims {
    int64_t max_blocks, max_pixels;
    int max_intervals;
};

// everything the kernels index with, checked on the host copy of the plans
int check_plans(const hoig_jpeg_plan *plans, int n, int64_t nbytes, int64_t n_entries, bool entropy, int64_t out_bytes,
                int64_t workspace_bytes, BatchDims *d) {
    d->max_blocks = d->max_pixels = 0;
    d->max_intervals = 0;
    for (int i = 0; i < n; ++i) {
        const hoig_jpeg_plan &P = plans[i];
        if (!jpeg_plan_sane(P)) return HOIG_EUNSUPPORTED;
        const int64_t blocks = jpeg_geometry(P).blocks, pixels = (int64_t)P.width * P.height;
        if (entropy && (P.data_off + P.data_len > nbytes || (int64_t)P.interval_first + P.n_intervals + 1 > n_entries)) return HOIG_EINVAL;
        if (P.coef_off < 0 || P.coef_off % 16 || P.coef_off + blocks * 128 > workspace_bytes) return HOIG_EINVAL;
        if (P.plane_off < 0 || P.plane_off % 8 || P.plane_off + blocks * 64 > workspace_bytes) return HOIG_EINVAL;
        if (P.out_off < 0 || P.out_off + pixels * 3 > out_bytes) return HOIG_EINVAL;
        d->max_blocks = blocks > d->max_blocks ? blocks : d->max_blocks;
        d->max_pixels = pixels > d->max_pixels ? pixels : d->max_pixels;
        d->max_intervals = P.n_intervals > d->max_intervals ? P.n_intervals : d->max_intervals;
    }
    return HOIG_OK;
}

int reconstruct(const hoig_jpeg_plan *plans_dev, int n, const BatchDims &d, uint8_t *out, void *workspace, hipStream_t stream) {
    jpeg_idct_kernel<<<dim3(hoig_stream_grid(d.max_blocks, 256), n), 256, 0, stream>>>(plans_dev, static_cast<char *>(workspace));
    HOIG_LAUNCH_CHECK();
    jpeg_colour_kernel<<<dim3(hoig_stream_grid(d.max_pixels, 256), n), 256, 0, stream>>>(plans_dev, static_cast<const char *>(workspace), out);
    HOIG_LAUNCH_CHECK();
    return HOIG_OK;
}

}  // namespace

extern "C" int hoig_jpeg_decode_bgr_u8(const uint8_t *bytes, int64_t nbytes, const hoig_jpeg_plan *plans_host,
                                       const hoig_jpeg_plan *plans_dev, int n, const int32_t *intervals, int64_t n_entries, uint8_t *out,
                                       int64_t out_bytes, int32_t *status, void *workspace, int64_t workspace_bytes, hoig_stream_t stream) {
    if (!bytes || !plans_host || !plans_dev || !intervals || !out || !status || !workspace || n <= 0 || n > 65535) return HOIG_EINVAL;
    if (nbytes <= 0 || nbytes % 16 || ((uintptr_t)bytes & 15) || ((uintptr_t)workspace & 15)) return HOIG_EINVAL;
    BatchDims d;
    const int rc = check_plans(plans_host, n, nbytes, n_entries, true, out_bytes, workspace_bytes, &d);
    if (rc != HOIG_OK) return rc;
    if (hipMemsetAsync(status, 0, sizeof(int32_t) * n, (hipStream_t)stream) != hipSuccess) return HOIG_ELAUNCH;
    jpeg_entropy_kernel<<<dim3(d.max_intervals, n), 64, 0, (hipStream_t)stream>>>(bytes, nbytes, plans_dev, intervals, status,
                                                                                 static_cast<char *>(workspace));
    HOIG_LAUNCH_CHECK();
    return reconstruct(plans_dev, n, d, out, workspace, (hipStream_t)stream);
}

extern "C" int hoig_jpeg_reconstruct_bgr_u8(const hoig_jpeg_plan *plans_host, const hoig_jpeg_plan *plans_dev, int n, uint8_t *out,
                                            int64_t out_bytes, void *workspace, int64_t workspace_bytes, hoig_stream_t stream) {
    if (!plans_host || !plans_dev || !out || !workspace || n <= 0 || n > 65535 || ((uintptr_t)workspace & 15)) return HOIG_EINVAL;
    BatchDims d;
    const int rc = check_plans(plans_host, n, 0, 0, false, out_bytes, workspace_bytes, &d);
    if (rc != HOIG_OK) return rc;
    return reconstruct(plans_dev, n, d, out, workspace, (hipStream_t)stream);
}

extern "C" int hoig_jpeg_decode_bgr_u8_par(const uint8_t *bytes, int64_t nbytes, const hoig_jpeg_plan *plans_host,
                                           const hoig_jpeg_plan *plans_dev, int n, const int32_t *intervals, int64_t n_entries,
                                           uint8_t *out, int64_t out_bytes, int32_t *status, void *workspace, int64_t workspace_bytes,
                                           int subseq_bytes, hoig_stream_t stream) {
    if (!bytes || !plans_host || !plans_dev || !intervals || !out || !status || !workspace || n <= 0 || n > 65535) return HOIG_EINVAL;
    if (nbytes <= 0 || nbytes % 16 || ((uintptr_t)bytes & 15) || ((uintptr_t)workspace & 15)) return HOIG_EINVAL;
    const int S = subseq_bytes ? subseq_bytes : HOIG_JPEG_SUBSEQ_BYTES;
    if (!jpeg_par_subseq_ok(S)) return HOIG_EINVAL;
    BatchDims d;
    const int rc = check_plans(plans_host, n, nbytes, n_entries, true, out_bytes, workspace_bytes, &d);
    if (rc != HOIG_OK) return rc;
    // the table of irregular intervals lies behind every plane, and the coefficients (zeroed here) in front of every plane
    int64_t tables, entries, coef_end = 0, plane_first = workspace_bytes;
    jpeg_par_tables(plans_host, n, &tables, &entries);
    if (tables + entries * (int64_t)sizeof(int32_t) > workspace_bytes) return HOIG_EINVAL;
    for (int i = 0; i < n; ++i) {
        const int64_t e = plans_host[i].coef_off + jpeg_geometry(plans_host[i]).blocks * 128;
        coef_end = e > coef_end ? e : coef_end;
        plane_first = plans_host[i].plane_off < plane_first ? plans_host[i].plane_off : plane_first;
    }
    if (coef_end > plane_first) return HOIG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char *work = static_cast<char *>(workspace);
    int32_t *irregular = reinterpret_cast<int32_t *>(work + tables);
    if (hipMemsetAsync(status, 0, sizeof(int32_t) * n, st) != hipSuccess) return HOIG_ELAUNCH;
    if (hipMemsetAsync(work, 0, (size_t)coef_end, st) != hipSuccess) return HOIG_ELAUNCH;
    int logs = 5;
    while ((1 << logs) < S) ++logs;
    const dim3 grid(d.max_intervals, n);
    if (S == 256) jpeg_entropy_par_kernel<128><<<grid, 128, 0, st>>>(bytes, nbytes, plans_dev, intervals, S, logs, irregular, work);
    else if (S == 128) jpeg_entropy_par_kernel<256><<<grid, 256, 0, st>>>(bytes, nbytes, plans_dev, intervals, S, logs, irregular, work);
    else jpeg_entropy_par_kernel<512><<<grid, 512, 0, st>>>(bytes, nbytes, plans_dev, intervals, S, logs, irregular, work);
    HOIG_LAUNCH_CHECK();
    jpeg_entropy_flagged_kernel<<<dim3(d.max_intervals, n), 64, 0, st>>>(bytes, nbytes, plans_dev, intervals, irregular, status, work);
    HOIG_LAUNCH_CHECK();
    return reconstruct(plans_dev, n, d, out, workspace, st);
}
