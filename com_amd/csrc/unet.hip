// The elementwise passes of UNetV2's UR block (pcdet/models/backbones_3d/spconv_unet.py:135-160) and its point outputs
// (:206-211) for gfx950.  UR_block_forward computes inv(relu(bn(conv_m(cat(b, t)))) + reduce(cat(b, t))) with
// reduce(c)[j] = c[2j] + c[2j+1]; here that is
//   merge_cat        cat [n][2C] from bottom [n][C] and trans [n][C]                       (instead of torch.cat)
//   bn_pairadd       out[j] = round(relu(x[j]*scale[j] + shift[j]) + (cat[2j] + cat[2j+1]))  (relu(bn(.)) never stored)
//   merge_backward   d_bottom[c] = d_cat[c] + dy[c >> 1],  d_trans[c] = d_cat[C + c] + dy[(C + c) >> 1]
//   point_outputs    point_coords = (b, (idx + 0.5) * voxel_size + range_min), padding rows behind a device row count
// All four: 16-byte pieces, grid-stride, fp32 arithmetic with one rounding to the storage type, rows behind *n_dev neither
// read nor (but for point_outputs' padding contract) written.
#include "common.h"

namespace {

constexpr int MID_ROWS = PCD_BN_MID_ROWS;
constexpr int MAX_BLOCKS = 2048;
constexpr int PPT = 4;   // pieces per thread the grid aims at

template <typename T>
struct Pc;
template <>
struct Pc<float> {
    static constexpr int N = 4;
    __device__ static void load(const float *p, float (&v)[4]) {
        const float4 r = *reinterpret_cast<const float4 *>(p);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    }
    __device__ static void load_half(const float *p, float (&v)[2]) {
        const float2 r = *reinterpret_cast<const float2 *>(p);
        v[0] = r.x; v[1] = r.y;
    }
    __device__ static void store(float *p, const float (&v)[4]) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};
template <>
struct Pc<unsigned short> {
    static constexpr int N = 8;
    __device__ static void load(const unsigned short *p, float (&v)[8]) {
        const uint4 r = *reinterpret_cast<const uint4 *>(p);
        const u32 w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __uint_as_float(w[j] << 16);
            v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
        }
    }
    __device__ static void load_half(const unsigned short *p, float (&v)[4]) {
        const uint2 r = *reinterpret_cast<const uint2 *>(p);
        v[0] = __uint_as_float(r.x << 16);
        v[1] = __uint_as_float(r.x & 0xffff0000u);
        v[2] = __uint_as_float(r.y << 16);
        v[3] = __uint_as_float(r.y & 0xffff0000u);
    }
    __device__ static void store(unsigned short *p, const float (&v)[8]) {
        u32 w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            w[j] = (u32)f32_to_bf16_bits(v[2 * j]) | ((u32)f32_to_bf16_bits(v[2 * j + 1]) << 16);
        *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
};

static int grid_for(size_t pieces) {
    size_t blocks = (pieces + (size_t)256 * PPT - 1) / ((size_t)256 * PPT);
    if (blocks > (size_t)MAX_BLOCKS) blocks = MAX_BLOCKS;
    return blocks < 1 ? 1 : (int)blocks;
}

// pieces per row of a [n][c] matrix, or 0 when the passes here do not serve the width (256 threads must hold whole rows)
static int row_pieces(int c, int dtype) {
    if (dtype != PCD_F32 && dtype != PCD_BF16) return 0;
    const int N = dtype == PCD_F32 ? 4 : 8;
    if (c <= 0 || c % N) return 0;
    const int pcs = c / N;
    return (pcs <= 256 && 256 % pcs == 0) ? pcs : 0;
}

static bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr) {
    const void *ps[4] = {a, b, c, d};
    for (const void *q : ps)
        if (q && ((uintptr_t)q & 15u)) return false;
    return true;
}

// cat[r][0..C) = bottom[r], cat[r][C..2C) = trans[r]: a copy of 16-byte pieces, `pcs` of them per input row
__global__ __launch_bounds__(256) void merge_cat_kernel(const uint4 *__restrict__ bottom, const uint4 *__restrict__ trans,
                                                        int n_cap, const int32_t *n_dev, int pcs, uint4 *__restrict__ cat) {
    const size_t total = (size_t)eff_rows(n_dev, n_cap) * 2 * pcs;
    const size_t S = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += S) {
        const size_t row = e / (2 * pcs);
        const int p = (int)(e - row * 2 * pcs);
        cat[e] = p < pcs ? bottom[row * pcs + p] : trans[row * pcs + (p - pcs)];
    }
}

struct PairAddStats {
    const double *mid;                       // training: [MID_ROWS][2][c] column sums (sum x, sum x^2); NULL: running stats
    const float *gamma, *beta;
    float eps, momentum;
    float *running_mean, *running_var, *save_mean, *save_invstd;
};

// out[r][j] = relu(x[r][j] * scale[j] + shift[j]) + (cat[r][2j] + cat[r][2j+1]); the statistics are finished from `mid` by
// every workgroup (workgroup 0 publishes them) in the arithmetic of the BatchNorm apply pass of fused.hip, so the backward
// pass of that BatchNorm, which recomputes the ReLU mask from x, sees the same signs.
template <typename T>
__global__ __launch_bounds__(256) void bn_pairadd_kernel(const T *__restrict__ x, const T *__restrict__ cat, int n_cap,
                                                         const int32_t *n_dev, int c, PairAddStats st, T *__restrict__ out) {
    constexpr int N = Pc<T>::N;
    extern __shared__ __attribute__((aligned(16))) char dyn_lds[];
    double *tot = (double *)dyn_lds;
    float *sc_s = (float *)(tot + 2 * c), *sh_s = sc_s + c;
    const int pcs = c / N;
    const int n = eff_rows(n_dev, n_cap);
    if (st.mid) {
        const int cols = 2 * c;
        for (int t = threadIdx.x; t < cols; t += (int)blockDim.x) {
            double v[MID_ROWS];
#pragma unroll
            for (int r = 0; r < MID_ROWS; ++r) v[r] = st.mid[(size_t)r * cols + t];
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < MID_ROWS; ++r) s += v[r];
            tot[t] = s;
        }
        __syncthreads();
    }
    for (int ch = threadIdx.x; ch < c; ch += (int)blockDim.x) {
        const float g = st.gamma ? st.gamma[ch] : 1.0f, b = st.beta ? st.beta[ch] : 0.0f;
        if (st.mid) {
            const double s = tot[ch], ss = tot[c + ch];
            double mean = n > 0 ? s / n : 0.0;
            double var = n > 0 ? ss / n - mean * mean : 0.0;
            if (var < 0.0) var = 0.0;
            const float invstd = (float)(1.0 / sqrt(var + (double)st.eps));
            sc_s[ch] = g * invstd;
            sh_s[ch] = b - (float)mean * g * invstd;
            if (blockIdx.x == 0) {
                st.save_mean[ch] = (float)mean;
                st.save_invstd[ch] = invstd;
                if (st.running_mean)
                    st.running_mean[ch] = (1.0f - st.momentum) * st.running_mean[ch] + st.momentum * (float)mean;
                if (st.running_var) {
                    const double unbiased = n > 1 ? var * (double)n / (double)(n - 1) : var;
                    st.running_var[ch] = (1.0f - st.momentum) * st.running_var[ch] + st.momentum * (float)unbiased;
                }
            }
        } else {
            const float invstd = 1.0f / sqrtf(st.running_var[ch] + st.eps);
            sc_s[ch] = g * invstd;
            sh_s[ch] = b - st.running_mean[ch] * g * invstd;
        }
    }
    __syncthreads();
    const size_t e0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, S = (size_t)gridDim.x * blockDim.x;
    const int piece = (int)(e0 % pcs);       // fixed: 256 and therefore S are multiples of pcs
    float sc[N], sh[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        sc[j] = sc_s[piece * N + j];
        sh[j] = sh_s[piece * N + j];
    }
    const size_t total = (size_t)n * pcs;
    for (size_t e = e0; e < total; e += S) {
        float v[N], lo[N], hi[N];
        Pc<T>::load(x + e * N, v);
        Pc<T>::load(cat + e * 2 * N, lo);        // row * 2c + piece * 2N = 2 * e * N
        Pc<T>::load(cat + e * 2 * N + N, hi);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            float o = v[j] * sc[j] + sh[j];
            o = o > 0.0f ? o : 0.0f;
            const float a = 2 * j < N ? lo[2 * j] : hi[2 * j - N];
            const float b = 2 * j < N ? lo[2 * j + 1] : hi[2 * j + 1 - N];
            v[j] = o + (a + b);
        }
        Pc<T>::store(out + e * N, v);
    }
}

// one thread per 16-byte piece q of the virtual row [2C] of d_cat: its N channels take dy's N / 2 channels q * N / 2 ...
template <typename T>
__global__ __launch_bounds__(256) void merge_backward_kernel(const T *__restrict__ d_cat, const T *__restrict__ dy, int n_cap,
                                                             const int32_t *n_dev, int c, T *__restrict__ d_bottom,
                                                             T *__restrict__ d_trans) {
    constexpr int N = Pc<T>::N;
    const int pcs = c / N;
    const size_t total = (size_t)eff_rows(n_dev, n_cap) * 2 * pcs;
    const size_t S = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += S) {
        const size_t row = e / (2 * pcs);
        const int p = (int)(e - row * 2 * pcs);
        float g[N], h[N / 2];
        Pc<T>::load(d_cat + e * N, g);
        Pc<T>::load_half(dy + row * c + (size_t)p * (N / 2), h);
#pragma unroll
        for (int j = 0; j < N; ++j) g[j] = g[j] + h[j >> 1];
        T *dst = p < pcs ? d_bottom + row * c + (size_t)p * N : d_trans + row * c + (size_t)(p - pcs) * N;
        Pc<T>::store(dst, g);
    }
}

// dst[b][k][a] = src[a][k][b]: the class weight gradient of a strided conv run with its two operands swapped leaves the
// inverse conv's dU transposed (src = [cin][K][cout] of the inverse conv, dst = its parameter layout [cout][K][cin])
__global__ __launch_bounds__(256) void transpose_wgrad_kernel(const float *__restrict__ src, int a_n, int k_n, int b_n,
                                                              float *__restrict__ dst) {
    const size_t total = (size_t)a_n * k_n * b_n;
    const size_t S = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += S) {
        // e indexes dst (coalesced writes): e = (b k_n + k) a_n + a
        const size_t a = e % a_n, t = e / a_n;
        const size_t k = t % k_n, b = t / k_n;
        dst[e] = src[(a * k_n + k) * b_n + b];
    }
}

struct PointGeom {
    float vx, vy, vz, x0, y0, z0;
};

// indices [n][4] = (b, z, y, x) -> coords [cap][4] = (b, cx, cy, cz); rows [n, cap): coords (-1, 0, 0, 0) and, with
// `features` ([cap] rows of feat_pieces 16-byte pieces), zeros there.  coords == NULL: the feature rows only.
__global__ __launch_bounds__(256) void point_outputs_kernel(const int4 *__restrict__ indices, int n_cap, const int32_t *n_dev,
                                                            PointGeom g, float4 *__restrict__ coords,
                                                            uint4 *__restrict__ features, int feat_pieces) {
    const int n = eff_rows(n_dev, n_cap);
    const size_t S = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < (size_t)n_cap; r += S) {
        if (r < (size_t)n) {
            if (!coords) continue;
            const int4 v = indices[r];
            float4 o;
            o.x = (float)v.x;
            // (idx + 0.5) * voxel_size + range_min: product and sum rounded separately, as torch's two kernels do
            o.y = __fadd_rn(__fmul_rn(__fadd_rn((float)v.w, 0.5f), g.vx), g.x0);
            o.z = __fadd_rn(__fmul_rn(__fadd_rn((float)v.z, 0.5f), g.vy), g.y0);
            o.w = __fadd_rn(__fmul_rn(__fadd_rn((float)v.y, 0.5f), g.vz), g.z0);
            coords[r] = o;
        } else if (n_dev) {
            if (coords) coords[r] = make_float4(-1.0f, 0.0f, 0.0f, 0.0f);
            if (features)
                for (int p = 0; p < feat_pieces; ++p) features[r * feat_pieces + p] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

}  // namespace

extern "C" int pcd_unet_merge_cat(const void *bottom, const void *trans, int dtype, int n, int c, const int32_t *n_dev,
                                  void *cat, void *stream) {
    PCD_ENTER();
    if (n < 0) return PCD_ERR_INVALID_ARG;
    const int pcs = row_pieces(c, dtype);
    if (!pcs) return PCD_ERR_UNSUPPORTED;
    if (n == 0) return PCD_OK;
    if (!bottom || !trans || !cat || !aligned16(bottom, trans, cat)) return PCD_ERR_INVALID_ARG;
    merge_cat_kernel<<<grid_for((size_t)n * 2 * pcs), 256, 0, (hipStream_t)stream>>>((const uint4 *)bottom, (const uint4 *)trans,
                                                                                      n, n_dev, pcs, (uint4 *)cat);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_unet_bn_pairadd(const void *x, const void *cat, int dtype, int n, int c, const float *gamma,
                                   const float *beta, float eps, float momentum, const double *mid, float *running_mean,
                                   float *running_var, float *save_mean, float *save_invstd, const int32_t *n_dev, void *out,
                                   void *stream) {
    PCD_ENTER();
    if (n < 0) return PCD_ERR_INVALID_ARG;
    const int pcs = row_pieces(c, dtype);
    if (!pcs || c > 1024) return PCD_ERR_UNSUPPORTED;
    if (mid ? (!save_mean || !save_invstd) : (!running_mean || !running_var)) return PCD_ERR_INVALID_ARG;
    if (n == 0) return PCD_OK;
    if (!x || !cat || !out || !aligned16(x, cat, out)) return PCD_ERR_INVALID_ARG;
    PairAddStats st = {mid, gamma, beta, eps, momentum, running_mean, running_var, save_mean, save_invstd};
    if (!mid) st.save_mean = st.save_invstd = nullptr;
    const size_t lds = (size_t)2 * c * sizeof(double) + (size_t)2 * c * sizeof(float);
    const int grid = grid_for((size_t)n * pcs);
    if (dtype == PCD_F32)
        bn_pairadd_kernel<float><<<grid, 256, lds, (hipStream_t)stream>>>((const float *)x, (const float *)cat, n, n_dev, c, st,
                                                                         (float *)out);
    else
        bn_pairadd_kernel<unsigned short><<<grid, 256, lds, (hipStream_t)stream>>>(
            (const unsigned short *)x, (const unsigned short *)cat, n, n_dev, c, st, (unsigned short *)out);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_unet_merge_backward(const void *d_cat, const void *dy, int dtype, int n, int c, const int32_t *n_dev,
                                       void *d_bottom, void *d_trans, void *stream) {
    PCD_ENTER();
    if (n < 0) return PCD_ERR_INVALID_ARG;
    const int pcs = row_pieces(c, dtype);
    if (!pcs) return PCD_ERR_UNSUPPORTED;
    if (n == 0) return PCD_OK;
    if (!d_cat || !dy || !d_bottom || !d_trans || !aligned16(d_cat, dy, d_bottom, d_trans)) return PCD_ERR_INVALID_ARG;
    const int grid = grid_for((size_t)n * 2 * pcs);
    if (dtype == PCD_F32)
        merge_backward_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float *)d_cat, (const float *)dy, n, n_dev, c,
                                                                           (float *)d_bottom, (float *)d_trans);
    else
        merge_backward_kernel<unsigned short><<<grid, 256, 0, (hipStream_t)stream>>>(
            (const unsigned short *)d_cat, (const unsigned short *)dy, n, n_dev, c, (unsigned short *)d_bottom,
            (unsigned short *)d_trans);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_unet_point_outputs(const int32_t *indices, int n, const int32_t *n_dev, float vx, float vy, float vz,
                                      float x0, float y0, float z0, float *coords, void *features, int feature_row_bytes,
                                      void *stream) {
    PCD_ENTER();
    if (n < 0 || feature_row_bytes < 0 || feature_row_bytes % 16) return PCD_ERR_INVALID_ARG;
    if (n == 0) return PCD_OK;
    if ((coords ? !indices : !(features && n_dev)) || !aligned16(indices, coords, features)) return PCD_ERR_INVALID_ARG;
    const PointGeom g = {vx, vy, vz, x0, y0, z0};
    int grid = (n + 255) / 256;
    if (grid > MAX_BLOCKS) grid = MAX_BLOCKS;
    point_outputs_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const int4 *)indices, n, n_dev, g, (float4 *)coords,
                                                               (uint4 *)features, feature_row_bytes / 16);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_unet_transpose_wgrad(const float *src, int cin, int kvol, int cout, float *dst, void *stream) {
    PCD_ENTER();
    if (cin <= 0 || kvol <= 0 || cout <= 0 || !src || !dst || src == dst) return PCD_ERR_INVALID_ARG;
    transpose_wgrad_kernel<<<grid_for((size_t)cin * kvol * cout), 256, 0, (hipStream_t)stream>>>(src, cin, kvol, cout, dst);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
