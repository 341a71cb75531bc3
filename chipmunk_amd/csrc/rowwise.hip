// Row-wise passes of the transformer block around the attention / MLP operators (model code in the reference, torch ops there):
// gated residual + LayerNorm + modulate in one pass over the hidden state; block means; fp8 input quantisation; Wan's row-wide q / k
// RMSNorm + rotary + head-major layout (split_heads_rownorm_kernel, at the end of the file).
//
// The blocks of the DiT models the reference patches do, between any two GEMMs,
//     x  = x + gate * y                      (torch.addcmul; examples/hunyuan/hyvideo/modules/models.py:262-275, 431)
//     xm = LayerNorm(x) * (1 + scale) + shift   (modulate(norm(x)), models.py:184-186, 265-268, 371-372; no affine, eps 1e-6)
// as three elementwise / normalisation kernels: 8 passes over the [rows, C] bf16 hidden state (read x, y, write x; read x, write
// xn; read xn, write xm) where 4 suffice (read x, y; write x, xm).  HBM-bound: 4 * rows * C * 2 bytes per call.
//
// One wave per row (C = 3 072: 6 x 16 bytes per lane), the row in registers between the two reductions (mean, then the centred
// sum of squares: the two-pass form, no E[x^2] - E[x]^2 cancellation), 64-lane sums by DPP + lane swaps, no LDS.  A wave keeps
// its gate / shift / scale vectors in registers and walks rows with the grid's stride.  Rounding points are torch's: bf16 after
// the residual, bf16 after the normalisation, bf16(1 + scale), bf16 after the modulation.
#include "common.h"

namespace {

template <int NV, bool RESIDUAL>   // NV 16-byte vectors per lane: C <= 512 * NV
__global__ __launch_bounds__(256) void residual_ln_modulate_kernel(const uint16_t *x, const uint16_t *y, const uint16_t *gate,
                                                                   const uint16_t *shift, const uint16_t *scale, uint16_t *x_out,
                                                                   uint16_t *xm, int64_t rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const float inv_c = 1.0f / (float)C;
    u32x4 g[NV], sh[NV], sc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = (lane + 64 * j) * 8;
        const u32x4 z = {0u, 0u, 0u, 0u};
        g[j] = (RESIDUAL && c < C) ? *(const u32x4 *)(gate + c) : z;
        sh[j] = c < C ? *(const u32x4 *)(shift + c) : z;
        sc[j] = c < C ? *(const u32x4 *)(scale + c) : z;
#pragma unroll
        for (int e = 0; e < 4; ++e) {   // bf16(1 + scale), once per wave
            float a = 1.0f + __uint_as_float(sc[j][e] << 16), b = 1.0f + __uint_as_float(sc[j][e] & 0xffff0000u);
            sc[j][e] = pack_bf16x2(a, b);
        }
    }
    for (int64_t r = wave; r < rows; r += nwaves) {
        float f[NV][8];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = (lane + 64 * j) * 8;
            u32x4 xv = {0u, 0u, 0u, 0u}, yv = xv;
            if (c < C) {
                xv = *(const u32x4 *)(x + r * C + c);
                if constexpr (RESIDUAL) yv = *(const u32x4 *)(y + r * C + c);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = __uint_as_float(xv[e] << 16), b = __uint_as_float(xv[e] & 0xffff0000u);
                if constexpr (RESIDUAL) {
                    a += __uint_as_float(g[j][e] << 16) * __uint_as_float(yv[e] << 16);
                    b += __uint_as_float(g[j][e] & 0xffff0000u) * __uint_as_float(yv[e] & 0xffff0000u);
                    round_bf16_pair(a, b);
                    xv[e] = pack_bf16x2(a, b);
                }
                f[j][2 * e] = a, f[j][2 * e + 1] = b;
                sum += a + b;
            }
            if constexpr (RESIDUAL)
                if (c < C) *(u32x4 *)(x_out + r * C + c) = xv;
        }
        const float mean = sum_across_rows(row16_sum(sum)) * inv_c;
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const bool in = (lane + 64 * j) * 8 < C;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                f[j][e] -= mean;
                ss = in ? __builtin_fmaf(f[j][e], f[j][e], ss) : ss;
            }
        }
        const float var = sum_across_rows(row16_sum(ss)) * inv_c;
        const float rstd = 1.0f / __builtin_sqrtf(var + eps);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = (lane + 64 * j) * 8;
            u32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = f[j][2 * e] * rstd, b = f[j][2 * e + 1] * rstd;
                round_bf16_pair(a, b);
                a = __builtin_fmaf(a, __uint_as_float(sc[j][e] << 16), __uint_as_float(sh[j][e] << 16));
                b = __builtin_fmaf(b, __uint_as_float(sc[j][e] & 0xffff0000u), __uint_as_float(sh[j][e] & 0xffff0000u));
                o[e] = pack_bf16x2(a, b);
            }
            if (c < C) *(u32x4 *)(xm + r * C + c) = o;
        }
    }
}

template <int NV>
void launch_rlm(const void *x, const void *y, const void *gate, const void *shift, const void *scale, void *x_out, void *xm, int64_t rows,
                int C, float eps, hipStream_t s) {
    // 4 rows per workgroup at a time; enough workgroups for 8 per CU, the rest of the rows by stride
    const int64_t want = (rows + 3) / 4;
    const unsigned grid = (unsigned)(want < 256 * 8 ? want : 256 * 8);
    if (y)
        hipLaunchKernelGGL((residual_ln_modulate_kernel<NV, true>), dim3(grid), dim3(256), 0, s, (const uint16_t *)x, (const uint16_t *)y,
                           (const uint16_t *)gate, (const uint16_t *)shift, (const uint16_t *)scale, (uint16_t *)x_out, (uint16_t *)xm, rows,
                           C, eps);
    else
        hipLaunchKernelGGL((residual_ln_modulate_kernel<NV, false>), dim3(grid), dim3(256), 0, s, (const uint16_t *)x, nullptr, nullptr,
                           (const uint16_t *)shift, (const uint16_t *)scale, nullptr, (uint16_t *)xm, rows, C, eps);
}


// Mean over consecutive blocks of `mbm` rows: [R, C] -> [R / mbm, C] bf16 (reference modules/mlp.py:11-16, `block_mean`, the first
// operation of every sparse MLP step; torch's reshape + mean kernel reads the 27 MB of a FLUX layer's input in 17 us).  One workgroup
// = (block, 512 columns): the four waves take a quarter of the block's rows each, a lane 8 columns (16 bytes) of every row; fp32
// sums in row order, the four partial sums added in wave order, one rounding to bf16.  HBM-bound: R * C * 2 bytes.
// A ragged last block (R % mbm != 0) is the mean over the rows present: every wave keeps its slice of the block and stops at row R.
template <int NW, int VEC>   // NW waves per workgroup, each takes mbm / NW rows of the block (all requested before the first is added);
__global__ __launch_bounds__(NW * 64) void block_mean_kernel(const uint16_t *x, uint16_t *out, int64_t rows, int C, int mbm) {   // VEC = columns per lane (8 or 4)
    __shared__ float part[NW - 1][64][VEC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * VEC;
    const int64_t blk = blockIdx.y;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    if (c < C) {
        const int per = mbm / NW;
        const int64_t first = blk * mbm + (int64_t)w * per;
        const int mine = (int)min((int64_t)per, max((int64_t)0, rows - first));   // rows of this wave's slice that exist
        const uint16_t *src = x + first * C + c;
#pragma unroll 16
        for (int r = 0; r < mine; ++r) {
            uint32_t v[VEC / 2];
            if constexpr (VEC == 8) {
                const u32x4 t = *(const u32x4 *)(src + (int64_t)r * C);
                v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
            } else {
                const u32x2 t = *(const u32x2 *)(src + (int64_t)r * C);
                v[0] = t[0], v[1] = t[1];
            }
#pragma unroll
            for (int e = 0; e < VEC / 2; ++e) acc[2 * e] += __uint_as_float(v[e] << 16), acc[2 * e + 1] += __uint_as_float(v[e] & 0xffff0000u);
        }
    }
    if (w > 0) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) part[w - 1][lane][e] = acc[e];
    }
    __syncthreads();
    if (w == 0 && c < C) {
        const float inv = 1.0f / (float)min((int64_t)mbm, rows - blk * mbm);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
#pragma unroll
            for (int ww = 0; ww < NW - 1; ++ww) acc[e] += part[ww][lane][e];      // fixed order: wave 0's rows, then waves 1 .. NW-1
        uint32_t o[VEC / 2];
#pragma unroll
        for (int e = 0; e < VEC / 2; ++e) o[e] = pack_bf16x2(acc[2 * e] * inv, acc[2 * e + 1] * inv);
        if constexpr (VEC == 8) *(u32x4 *)(out + blk * C + c) = (u32x4){o[0], o[1], o[2], o[3]};
        else *(u32x2 *)(out + blk * C + c) = (u32x2){o[0], o[1]};
    }
}
}  // namespace

extern "C" int chipmunk_residual_ln_modulate(const void *x, const void *y, const void *gate, const void *shift, const void *scale,
                                             void *x_out, void *xm, int64_t rows, int cols, double eps, void *stream) {
    CM_CHECK(x && shift && scale && xm, "residual_ln_modulate: null pointer");
    CM_CHECK((y == nullptr) == (gate == nullptr) && (y == nullptr) == (x_out == nullptr),
             "residual_ln_modulate: y, gate and x_out come together (all set: residual form; all null: LayerNorm + modulate only)");
    CM_CHECK(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 512 * 16, "residual_ln_modulate: cols must be a multiple of 8, at most 8192 (got %d)",
             cols);
    CM_CHECK(((((uintptr_t)x | (uintptr_t)y | (uintptr_t)gate | (uintptr_t)shift | (uintptr_t)scale | (uintptr_t)x_out | (uintptr_t)xm)) & 15) == 0,
             "residual_ln_modulate: pointers must be 16-byte aligned");
    if (rows == 0) return CHIPMUNK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int nv = (cols + 511) / 512;
    const float e = (float)eps;
    if (nv <= 2) launch_rlm<2>(x, y, gate, shift, scale, x_out, xm, rows, cols, e, s);
    else if (nv <= 3) launch_rlm<3>(x, y, gate, shift, scale, x_out, xm, rows, cols, e, s);
    else if (nv <= 6) launch_rlm<6>(x, y, gate, shift, scale, x_out, xm, rows, cols, e, s);
    else if (nv <= 10) launch_rlm<10>(x, y, gate, shift, scale, x_out, xm, rows, cols, e, s);
    else launch_rlm<16>(x, y, gate, shift, scale, x_out, xm, rows, cols, e, s);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

namespace {
int block_mean_entry(const void *x, void *out, int64_t rows, int C, int mbm, bool ragged, void *stream) {
    CM_CHECK(x && out, "block_mean: null tensor pointer");
    CM_CHECK(mbm > 0 && mbm % 4 == 0 && rows > 0 && (ragged || rows % mbm == 0),
             "block_mean: rows (%lld) must be a positive multiple of mbm (%d), mbm a multiple of 4", (long long)rows, mbm);
    const int64_t blocks = (rows + mbm - 1) / mbm;
    CM_CHECK(C > 0 && C % 8 == 0 && blocks < 65536, "block_mean: C must be a positive multiple of 8 and rows / mbm < 65536");
    // 8 waves x mbm / 8 rows x FOUR columns per lane when the block divides (FLUX / Wan: 128 rows): 408 workgroups instead of 204 and 16 loads in
    // flight per lane -- 27 MB of cold rows in 6.5 us (4.2 TB/s); 4 waves x 8 columns measured 17.3 us, 8 x 8: 10.9, 16 x 4: 7.3, 8 x 2: 6.5
    if (mbm % 8 == 0)
        hipLaunchKernelGGL((block_mean_kernel<8, 4>), dim3((C + 255) / 256, (unsigned)blocks), dim3(512), 0, (hipStream_t)stream,
                           (const uint16_t *)x, (uint16_t *)out, rows, C, mbm);
    else
        hipLaunchKernelGGL((block_mean_kernel<4, 8>), dim3((C + 511) / 512, (unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                           (const uint16_t *)x, (uint16_t *)out, rows, C, mbm);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}
}  // namespace

extern "C" int chipmunk_block_mean(const void *x, void *out, int64_t rows, int C, int mbm, void *stream) {
    return block_mean_entry(x, out, rows, C, mbm, false, stream);
}
extern "C" int chipmunk_block_mean_ragged(const void *x, void *out, int64_t rows, int C, int mbm, void *stream) {
    return block_mean_entry(x, out, rows, C, mbm, true, stream);
}

// ---------------------------------------------------------------------------------------------- fp8 input quantisation
// F8Linear.quantize_input (reference src/chipmunk/modules/mlp_fp8.py / flux fp8 linear: `(x * scale).clamp(-max, max).to(float8_e4m3fn)`)
// as ONE pass: torch runs it as three elementwise kernels (140 us at Wan2.1's 32 768 x 1536 rows, next to a 350 us GEMM1).  Same arithmetic,
// bit for bit: the scale is rounded to bf16 and the product formed in fp32 and rounded to bf16 (torch's bf16 tensor x 0-dim fp32 tensor), clamped in bf16 (NaN stays NaN), and
// converted to OCP e4m3 with round-to-nearest-even (v_cvt_pk_fp8_f32; the clamp keeps every value in range).
namespace {
__global__ __launch_bounds__(256) void quantize_fp8_kernel(const uint16_t *x, const float *scale, uint8_t *out, int64_t n8, float maxv) {
    // torch multiplies a bf16 tensor by a 0-dim fp32 tensor in the tensor's dtype: the scale is rounded to bf16 first
    const float sc = bf16_bits_to_f32(f32_to_bf16_bits(scale[0]));
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const u32x4 v = *(const u32x4 *)(x + i * 8);
        float f[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f[2 * e] = __uint_as_float(v[e] << 16) * sc;
            f[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u) * sc;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float r = bf16_bits_to_f32(f32_to_bf16_bits(f[e]));      // the bf16 product torch materialises
            r = r != r ? r : fminf(fmaxf(r, -maxv), maxv);           // clamp; NaN propagates as in torch
            f[e] = r;
        }
        u32x2 o;
        int w0 = 0, w1 = 0;
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false);
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
        o[0] = (uint32_t)w0, o[1] = (uint32_t)w1;
#pragma unroll
        for (int e = 0; e < 8; ++e)              // NaN: torch's cast gives 0x7f with the input's sign
            if (f[e] != f[e]) {
                const uint32_t byte = 0x7fu | ((__float_as_uint(f[e]) >> 24) & 0x80u);
                o[e >> 2] = (o[e >> 2] & ~(0xffu << ((e & 3) * 8))) | (byte << ((e & 3) * 8));
            }
        *(u32x2 *)(out + i * 8) = o;
    }
}
}  // namespace

extern "C" int chipmunk_quantize_fp8(const void *x, const float *scale, void *out, int64_t n, float max_value, void *stream) {
    CM_CHECK(x && scale && out, "quantize_fp8: null pointer");
    CM_CHECK(n >= 0 && n % 8 == 0, "quantize_fp8: the element count must be a multiple of 8 (got %lld)", (long long)n);
    CM_CHECK((((uintptr_t)x & 15) | ((uintptr_t)out & 7)) == 0, "quantize_fp8: x must be 16-byte and out 8-byte aligned");
    if (n == 0) return CHIPMUNK_OK;
    const int64_t n8 = n / 8;
    const int64_t blocks = (n8 + 255) / 256;
    hipLaunchKernelGGL(quantize_fp8_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t *)x, scale, (uint8_t *)out, n8, max_value);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

// ---------------------------------------------------------------------------------------------- fp8 input quantisation, one scale per row
// F8Linear.quantize_input_rowwise: per row r of a bf16 [rows, K] tensor, all in fp32 with IEEE division,
//     amax = max_k |x[r, k]|;  scale = min(max / max(amax, 1e-12), max);  out[r, k] = e4m3_rne(clamp(float(x[r, k]) * scale, -max, max));
//     scale_recip[r] = 1 / scale
// -- torch's `x.float() * scale[:, None]` chain: the product is fp32 and rounded ONCE, into e4m3 (the per-tensor kernel above mirrors
// torch's bf16 x 0-dim product and rounds to bf16 in between; this one does not).  One wave per row and one pass over HBM: the row stays
// packed in registers (NV 16-byte vectors per lane, K <= 512 * NV) between the |max| reduction (DPP + lane swaps, no LDS) and the
// conversion; a wave walks rows with the grid's stride.  HBM-bound: 3 * rows * K + 4 * rows bytes.  Rows with a NaN or Inf are outside the
// contract (amax, and with it every byte of the row, is then unspecified).
namespace {
__device__ __forceinline__ float row16_max(float x) {
    x = fmaxf(x, dpp_row_ror<8>(x));
    x = fmaxf(x, dpp_row_ror<4>(x));
    x = fmaxf(x, dpp_row_ror<2>(x));
    x = fmaxf(x, dpp_row_ror<1>(x));
    return x;
}

template <int NV>
__global__ __launch_bounds__(256) void quantize_fp8_rowwise_kernel(const uint16_t *x, uint8_t *out, float *scale_recip, int64_t rows, int K,
                                                                   float maxv) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t r = wave; r < rows; r += nwaves) {
        u32x4 xv[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = (lane + 64 * j) * 8;
            const u32x4 z = {0u, 0u, 0u, 0u};
            xv[j] = c < K ? *(const u32x4 *)(x + r * K + c) : z;   // (a vector past the row counts as zero: |0| changes no maximum)
        }
        float am = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                am = fmaxf(am, fmaxf(__uint_as_float((xv[j][e] << 16) & 0x7fffffffu), __uint_as_float(xv[j][e] & 0x7fff0000u)));
        am = max_across_rows(row16_max(am));
        const float scale = fminf(maxv / fmaxf(am, 1e-12f), maxv);   // amax_to_scale; IEEE division
        if (lane == 0) scale_recip[r] = 1.0f / scale;
        // the row stays packed across the reduction (see rownorm_rows: left alone the compiler keeps the unpacked floats, 8 per vector)
#pragma unroll
        for (int j = 0; j < NV; ++j) asm volatile("" : "+v"(xv[j]));
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = (lane + 64 * j) * 8;
            float f[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                f[2 * e] = fminf(fmaxf(__uint_as_float(xv[j][e] << 16) * scale, -maxv), maxv);
                f[2 * e + 1] = fminf(fmaxf(__uint_as_float(xv[j][e] & 0xffff0000u) * scale, -maxv), maxv);
            }
            int w0 = 0, w1 = 0;
            w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false);
            w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
            w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false);
            w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
            if (c < K) *(u32x2 *)(out + r * K + c) = (u32x2){(uint32_t)w0, (uint32_t)w1};
        }
    }
}

template <int NV>
void launch_quantize_rowwise(const void *x, void *out, float *scale_recip, int64_t rows, int K, float maxv, hipStream_t s) {
    // 4 rows per workgroup at a time; enough workgroups for 8 per CU, the rest of the rows by stride
    const int64_t want = (rows + 3) / 4;
    const unsigned grid = (unsigned)(want < 256 * 8 ? want : 256 * 8);
    hipLaunchKernelGGL((quantize_fp8_rowwise_kernel<NV>), dim3(grid), dim3(256), 0, s, (const uint16_t *)x, (uint8_t *)out, scale_recip, rows, K,
                       maxv);
}
}  // namespace

extern "C" int chipmunk_quantize_fp8_rowwise(const void *x, void *out, float *scale_recip, int64_t rows, int K, float max_value, void *stream) {
    CM_CHECK(x && out && scale_recip, "quantize_fp8_rowwise: null pointer");
    CM_CHECK(rows >= 0 && K > 0 && K % 16 == 0 && K <= CHIPMUNK_QUANTIZE_ROWWISE_MAX_K,
             "quantize_fp8_rowwise: K must be a positive multiple of 16, at most %d (got %d)", CHIPMUNK_QUANTIZE_ROWWISE_MAX_K, K);
    CM_CHECK(max_value > 0.f, "quantize_fp8_rowwise: max_value must be positive");
    CM_CHECK((((uintptr_t)x & 15) | ((uintptr_t)out & 7) | ((uintptr_t)scale_recip & 3)) == 0,
             "quantize_fp8_rowwise: x must be 16-byte, out 8-byte and scale_recip 4-byte aligned");
    if (rows == 0) return CHIPMUNK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int nv = (K + 511) / 512;
#define CM_QROW_CASE(NV) if (nv <= NV) { launch_quantize_rowwise<NV>(x, out, scale_recip, rows, K, max_value, s); } else
    CM_QROW_CASE(1) CM_QROW_CASE(2) CM_QROW_CASE(3) CM_QROW_CASE(4) CM_QROW_CASE(6) CM_QROW_CASE(8) CM_QROW_CASE(12) CM_QROW_CASE(16)
    CM_QROW_CASE(24) launch_quantize_rowwise<32>(x, out, scale_recip, rows, K, max_value, s);
#undef CM_QROW_CASE
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

// ---------------------------------------------------------------------------------------------- Wan attention operands
// Wan's blocks (reference examples/wan/wan/modules/model.py:81-97, 154-164, 195-196, 236-239) normalise q and k over the WHOLE
// projection row -- WanRMSNorm(dim), dim = heads * 128 channels, a dim-entry weight -- then rotate (rope_apply, :49-78: complex
// product in fp64, three-axis table), permute to [B, H, L, D] and cast to bf16 (:164): about ten torch passes per layer, two of
// them in fp64.  Here: one pass.  One wave per (batch, token, part) item; a part is one of up to three consecutive heads * 128
// column blocks of the row (q | k | v).  A lane owns the 16-byte pieces at columns (j * 64 + lane) * 8, j < NV = ceil(heads / 4):
// a 16-lane group is one head's 256-byte segment, four heads per iteration, the row in registers as packed bf16.  The sum of
// squares is a per-lane fp32 fma chain in column order, then row16_sum + sum_across_rows: a fixed order, and a row's result does
// not depend on which wave took it.  Rounding points are torch's: bf16(x * r) (.type_as, :94); a bf16 weight rounds the product
// to bf16, an fp32 weight keeps it in fp32 (torch's promotion); rotated or not, one rounding to bf16 at the end (:164).  The
// rotation of pair (2i, 2i+1) is lane-local (a lane holds 4 whole pairs) and evaluated in fp32; a lane's position inside its
// head is the same in every iteration (64 is a multiple of 16), so it reads its 8 cos + 8 sin values once per row.  A part
// that is neither normalised nor rotated is a bit copy (v).  The four waves of a workgroup take consecutive items, so the q and k
// of one token read the same table lines together.  No LDS; every global access is 16 bytes; stores are whole 256-byte head rows.
// HBM-bound: (read + write) 4 bytes per element + one read of the tables.
namespace {
struct RownormArgs {
    const uint16_t *x;
    int64_t batch_stride, row_stride;   // elements
    const void *w0, *w1, *w2;           // per part: nullptr, bf16 [heads * 128] or fp32 [heads * 128]
    uint16_t *o0, *o1, *o2;             // per part: [B, heads, n, 128]
    const float *fcos, *fsin;           // [rope_rows, 128]
    int64_t n, rows, rope_rows;         // rows = B * n
    int parts, heads;
    uint32_t norm_mask, rope_mask, fp32_mask;   // bit p: part p is normalised / rotated / has an fp32 weight
    float eps;
};

// (batch, token) of the rows a wave walks, row0 + i * step, without a 64-bit division per row
struct RowWalk {
    int64_t b, tok, b_step, tok_step, n;
    __device__ RowWalk(int64_t row0, int64_t step, int64_t n_) : b(row0 / n_), tok(row0 % n_), b_step(step / n_), tok_step(step % n_), n(n_) {}
    __device__ void next() {
        b += b_step, tok += tok_step;
        if (tok >= n) tok -= n, ++b;
    }
};

// A wave's rows of one part.  WK: the part's weight (0 none, 1 bf16, 2 fp32), in registers for all of the wave's rows, as
// residual_ln_modulate_kernel keeps its vectors.  NV = ceil(heads / 4) exactly, so only the last vector can lie past the row (heads not a
// multiple of 4): it reads the row's last vector instead -- every load is unconditional and they all issue together -- and counts
// as zero; its store alone is conditional (a condition on every store has the compiler sink the loads behind it, one wait each).
template <int NV, int WK>
__device__ __forceinline__ void rownorm_rows(const RownormArgs &a, int part, int64_t row0, int64_t row_step, const void *wp, uint16_t *out,
                                             bool normed, bool rope) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, hq = lane >> 4;
    const int H = a.heads, C = H * 128;
    const int64_t rows = a.rows, dstep = a.n * 512;   // dstep: four heads further
    const bool tail_in = (NV - 1) * 4 + hq < H;                   // NV = ceil(heads / 4): only the last vector can lie past the row
    int col[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) col[j] = min((j * 64 + lane) * 8, C - 8);
    constexpr bool HELD = WK == 1 || (WK == 2 && NV <= 10);   // fp32 weights of a longer row (8 registers per vector) are read per row instead
    u32x4 wb[WK == 1 ? NV : 1];
    f32x4 wf[WK == 2 && HELD ? NV : 1][2];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        if constexpr (WK == 1) wb[j] = *(const u32x4 *)((const uint16_t *)wp + col[j]);
        if constexpr (WK == 2 && HELD) wf[j][0] = *(const f32x4 *)((const float *)wp + col[j]), wf[j][1] = *(const f32x4 *)((const float *)wp + col[j] + 4);
    }
    RowWalk w(row0, row_step, a.n);
    for (int64_t row = row0; row < rows; row += row_step, w.next()) {
        const int64_t b = w.b, tok = w.tok;
        const uint16_t *src = a.x + b * a.batch_stride + tok * a.row_stride + (int64_t)part * C;
        uint16_t *dst = out + ((b * H + hq) * a.n + tok) * 128 + l15 * 8;
        const bool rotated = rope && tok < a.rope_rows;
        u32x4 xv[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) xv[j] = *(const u32x4 *)(src + col[j]);
        f32x4 c0 = {1.f, 1.f, 1.f, 1.f}, c1 = c0, s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
        if (rotated) {   // a lane's place in its head is the same for every j: its 8 cos + 8 sin values, once per row
            const float *pc = a.fcos + tok * 128 + l15 * 8, *ps = a.fsin + tok * 128 + l15 * 8;
            c0 = *(const f32x4 *)pc, c1 = *(const f32x4 *)(pc + 4), s0 = *(const f32x4 *)ps, s1 = *(const f32x4 *)(ps + 4);
        }
        float r = 1.0f;   // (a part that is not normalised: x * 1 and its rounding to bf16 are exact)
        if (normed) {
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const bool in = j < NV - 1 || tail_in;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float lo = __uint_as_float(xv[j][e] << 16), hi = __uint_as_float(xv[j][e] & 0xffff0000u);
                    ss = in ? __builtin_fmaf(hi, hi, __builtin_fmaf(lo, lo, ss)) : ss;
                }
            }
            ss = sum_across_rows(row16_sum(ss));
            r = 1.0f / __builtin_sqrtf(ss / (float)C + a.eps);   // (IEEE divide and sqrt: torch's mean and rsqrt on the host)
        }
        // Registers: the row stays packed (4 per vector) across the reduction, the bf16 weights stay packed across rows.  The empty
        // asm statements hide the values' origin, or the compiler keeps the unpacked floats instead: 8 per vector each, and spills.
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            asm volatile("" : "+v"(xv[j]));
            if constexpr (WK == 1) asm volatile("" : "+v"(wb[j]));
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            u32x4 o;
            f32x4 w2[2];
            if constexpr (WK == 2 && HELD) w2[0] = wf[j][0], w2[1] = wf[j][1];
            if constexpr (WK == 2 && !HELD) w2[0] = *(const f32x4 *)((const float *)wp + col[j]), w2[1] = *(const f32x4 *)((const float *)wp + col[j] + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float re = __uint_as_float(xv[j][e] << 16) * r, im = __uint_as_float(xv[j][e] & 0xffff0000u) * r;
                round_bf16_pair(re, im);                                    // .type_as(x)
                if constexpr (WK == 1) {                                    // bf16 * bf16: the product is rounded to bf16
                    re *= __uint_as_float(wb[j][e] << 16), im *= __uint_as_float(wb[j][e] & 0xffff0000u);
                    round_bf16_pair(re, im);
                }
                if constexpr (WK == 2) re *= w2[e >> 1][2 * (e & 1)], im *= w2[e >> 1][2 * (e & 1) + 1];   // bf16 * fp32 parameter: stays fp32
                // (re, im) -> (re * c - im * s, re * s + im * c); both table entries of a pair carry its angle
                const float c = e < 2 ? c0[2 * e] : c1[2 * e - 4], sn = e < 2 ? s0[2 * e] : s1[2 * e - 4];
                o[e] = rotated ? pack_bf16x2(re * c - im * sn, re * sn + im * c) : pack_bf16x2(re, im);
            }
            if (j < NV - 1 || tail_in) *(u32x4 *)(dst + j * dstep) = o;
            __builtin_amdgcn_sched_barrier(0);   // one vector at a time: left to itself the scheduler widens all NV at once and runs out of registers
        }
    }
}

template <int NV>   // NV 16-byte vectors per lane: heads in 4 * NV - 3 .. 4 * NV
__global__ __launch_bounds__(256) void split_heads_rownorm_kernel(const RownormArgs a) {
    // item = (row, part); the launch makes the number of waves a multiple of parts, so a wave stays with one part
    const int64_t wave = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const int part = (int)(wave % a.parts);
    const int64_t row0 = wave / a.parts, row_step = nwaves / a.parts;
    const void *wp = part == 0 ? a.w0 : part == 1 ? a.w1 : a.w2;
    uint16_t *out = part == 0 ? a.o0 : part == 1 ? a.o1 : a.o2;
    const bool normed = a.norm_mask >> part & 1, rope = a.rope_mask >> part & 1;
    if (!normed && !rope) {   // bit copy into the head-major layout
        const int lane = threadIdx.x & 63, l15 = lane & 15, hq = lane >> 4, H = a.heads;
        RowWalk w(row0, row_step, a.n);
        for (int64_t row = row0; row < a.rows; row += row_step, w.next()) {
            const int64_t b = w.b, tok = w.tok;
            const uint16_t *src = a.x + b * a.batch_stride + tok * a.row_stride + (int64_t)part * H * 128;
            uint16_t *dst = out + ((b * H + hq) * a.n + tok) * 128 + l15 * 8;
            u32x4 xv[NV];
#pragma unroll
            for (int j = 0; j < NV; ++j) xv[j] = *(const u32x4 *)(src + min((j * 64 + lane) * 8, H * 128 - 8));   // (see rownorm_rows)
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (j < NV - 1 || (NV - 1) * 4 + hq < H) *(u32x4 *)(dst + j * a.n * 512) = xv[j];
        }
    } else if (!wp) rownorm_rows<NV, 0>(a, part, row0, row_step, wp, out, normed, rope);
    else if (a.fp32_mask >> part & 1) rownorm_rows<NV, 2>(a, part, row0, row_step, wp, out, normed, rope);
    else rownorm_rows<NV, 1>(a, part, row0, row_step, wp, out, normed, rope);
}

template <int NV>
void launch_rownorm(const RownormArgs &a, hipStream_t s) {
    // 4 items per workgroup at a time; enough workgroups for 8 per CU, the rest of the items by stride; waves a multiple of parts
    int64_t grid = (a.rows * a.parts + 3) / 4;
    grid = grid < 256 * 8 ? grid : 256 * 8;
    if (a.parts == 3) grid = (grid + 2) / 3 * 3;
    hipLaunchKernelGGL((split_heads_rownorm_kernel<NV>), dim3((unsigned)grid), dim3(256), 0, s, a);
}
}  // namespace

extern "C" int chipmunk_split_heads_rownorm(const void *x, int64_t batch_stride, int64_t row_stride, int parts, const void *w0, int w0_dtype,
                                            const void *w1, int w1_dtype, const void *w2, int w2_dtype, void *out0, void *out1, void *out2,
                                            unsigned norm_mask, unsigned rope_mask, int64_t B, int64_t n, int heads, float eps,
                                            const float *freqs_cos, const float *freqs_sin, int64_t rope_rows, void *stream) {
    CM_CHECK(parts >= 1 && parts <= 3, "split_heads_rownorm: parts must be 1, 2 or 3 (got %d)", parts);
    CM_CHECK(heads >= 1 && heads <= 64, "split_heads_rownorm: heads must be in 1 .. 64 (got %d)", heads);
    CM_CHECK(B >= 1 && B < (1 << 24) && n >= 0 && n < ((int64_t)1 << 31), "split_heads_rownorm: B must be in 1 .. 2^24 - 1 and n in 0 .. 2^31 - 1 (got B=%lld n=%lld)",
             (long long)B, (long long)n);
    const void *w[3] = {w0, w1, w2};
    const int wd[3] = {w0_dtype, w1_dtype, w2_dtype};
    void *out[3] = {out0, out1, out2};
    CM_CHECK(x, "split_heads_rownorm: null input pointer");
    CM_CHECK((norm_mask >> parts) == 0 && (rope_mask >> parts) == 0, "split_heads_rownorm: norm_mask / rope_mask name a part past parts=%d", parts);
    uint32_t fp32_mask = 0;
    for (int p = 0; p < 3; ++p) {
        CM_CHECK(p >= parts || out[p], "split_heads_rownorm: null output pointer for part %d", p);
        CM_CHECK(wd[p] >= 0 && wd[p] <= 2 && (wd[p] == 0) == (w[p] == nullptr),
                 "split_heads_rownorm: weight %d: dtype code must be 0 (none, null pointer), 1 (bf16) or 2 (fp32)", p);
        CM_CHECK(wd[p] == 0 || (p < parts && (norm_mask >> p & 1)), "split_heads_rownorm: weight %d belongs to a part that is not normalised", p);
        if (wd[p] == 2) fp32_mask |= 1u << p;
    }
    CM_CHECK(row_stride >= (int64_t)parts * heads * 128 && batch_stride >= 0,
             "split_heads_rownorm: the row stride (%lld) must cover parts * heads * 128 = %lld columns", (long long)row_stride,
             (long long)parts * heads * 128);
    CM_CHECK((((uintptr_t)x | (uintptr_t)w0 | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)out0 | (uintptr_t)out1 | (uintptr_t)out2 |
               (uintptr_t)freqs_cos | (uintptr_t)freqs_sin) & 15) == 0 && (row_stride & 7) == 0 && (batch_stride & 7) == 0,
             "split_heads_rownorm: pointers must be 16-byte aligned, the batch and row strides multiples of 8 elements");
    CM_CHECK((freqs_cos == nullptr) == (freqs_sin == nullptr), "split_heads_rownorm: freqs_cos and freqs_sin come together (both or neither)");
    CM_CHECK(rope_mask == 0 || freqs_cos, "split_heads_rownorm: a rotated part needs freqs_cos / freqs_sin");
    CM_CHECK(rope_rows >= 0 && rope_rows <= n && (freqs_cos || rope_rows == 0), "split_heads_rownorm: rope_rows (%lld) must be in 0 .. n (%lld), 0 without tables",
             (long long)rope_rows, (long long)n);
    if (n == 0) return CHIPMUNK_OK;
    RownormArgs a;
    a.x = (const uint16_t *)x, a.batch_stride = batch_stride, a.row_stride = row_stride;
    a.w0 = w0, a.w1 = w1, a.w2 = w2;
    a.o0 = (uint16_t *)out0, a.o1 = (uint16_t *)out1, a.o2 = (uint16_t *)out2;
    a.fcos = freqs_cos, a.fsin = freqs_sin;
    a.n = n, a.rows = B * n, a.rope_rows = rope_rows;
    a.parts = parts, a.heads = heads;
    a.norm_mask = norm_mask, a.rope_mask = rope_rows > 0 ? rope_mask : 0u, a.fp32_mask = fp32_mask;
    a.eps = eps;
    hipStream_t s = (hipStream_t)stream;
    switch ((heads + 3) / 4) {
#define CM_ROWNORM_CASE(NV) case NV: launch_rownorm<NV>(a, s); break;
        CM_ROWNORM_CASE(1) CM_ROWNORM_CASE(2) CM_ROWNORM_CASE(3) CM_ROWNORM_CASE(4) CM_ROWNORM_CASE(5) CM_ROWNORM_CASE(6)
        CM_ROWNORM_CASE(7) CM_ROWNORM_CASE(8) CM_ROWNORM_CASE(9) CM_ROWNORM_CASE(10) CM_ROWNORM_CASE(11) CM_ROWNORM_CASE(12)
        CM_ROWNORM_CASE(13) CM_ROWNORM_CASE(14) CM_ROWNORM_CASE(15) CM_ROWNORM_CASE(16)
#undef CM_ROWNORM_CASE
    }
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

// ---------------------------------------------------------------------------------------------- Wan block glue
// Wan's blocks (reference examples/wan/wan/modules/model.py:317-334) keep the residual stream in fp32 and take their six modulation
// vectors as fp32 [B, 6, C], one set per SEQUENCE:
//     x  = x + y * e[2]                                   fp32 (:326-327, :333-334; `x + cross_attn(..)` without a gate, :331)
//     xm = norm(x).float() * (1 + e[1]) + e[0]            fp32, bf16 only at the next Linear (:324, :332)
//     xm = norm3(x)                                       LayerNorm with affine weight and bias (:283-285, :331)
// with WanLayerNorm = LayerNorm(x.float()).type_as(x) (:100-110) -- 3 - 5 torch kernels over an fp32 [B, L, C] stream per use.
// Here one pass: read x (fp32, or the bf16 of block 0) and y (bf16), write x_out (fp32) and xm (bf16): 12 bytes per element, 6 without y.
//
// As residual_ln_modulate_kernel above: one wave per row, the row in registers as fp32 between the two reductions (mean, then the
// centred sum of squares), row16_sum + sum_across_rows in a fixed order (a row's result does not depend on the wave that took it, nor on
// the batch it came in), no LDS, a wave walks rows with the grid's stride and RowWalk gives the row's sequence.  Rounding points are
// torch's: fp32(fp32(y) * gate), fp32(x + that) -- two operations, never a fused multiply-add --; for a bf16 x without y and with a
// modulation bf16(xn) (.type_as); then xm = bf16(fma(xn, mult, add)), mult = fp32(1 + scale) or the affine weight: ONE rounding.
//
// Lane-to-column mapping: a lane owns the 8 columns (lane + 64 j) * 8 .. + 7 of vector j, as everywhere in this file.  The bf16
// operands (y, xm, a bf16 x) are then one 16-byte access per lane and 1 KiB contiguous per wave instruction; an fp32 operand is the
// lane's 32 contiguous bytes as two 16-byte accesses issued back to back: each instruction touches every 128-byte line of the wave's
// 2 KiB span and takes half of it, the pair takes all of it, so every line is fetched from HBM once and wholly used while L1 serves
// two requests per line -- 32 useful bytes per L1 clock and CU, three times what a CU's share of HBM delivers.  The alternative (lane l
// reads fp32 columns 4 l .. 4 l + 3 of each 256-column half: 1 KiB contiguous per instruction) leaves a lane with two separate groups
// of 4 columns: 8-byte bf16 accesses, or a lane-pair exchange of 4 registers per load and store.  Not taken: the fp32 stream is the
// larger one but it is HBM, not L1, that bounds this kernel.
//
// The three fp32 vectors are 24 registers per row vector: HELD in registers where they fit beside the row (NV <= 6, C <= 3072: Wan
// 1.3B's 1536), re-read per row from L2 otherwise (C = 5120: 60 KB for the three, resident), the trade rownorm_rows makes.  Held
// vectors are re-read when the wave's row walk enters another sequence.
namespace {
struct GlueArgs {
    const void *x;                       // [rows, C] fp32 or bf16
    const uint16_t *y;                   // [rows, C] bf16 or nullptr
    const float *gate, *mult, *add;      // gate: nullptr = 1; mult: scale (modulation) or weight (affine); add: shift or bias
    float *x_out;                        // [rows, C] fp32 (with y)
    uint16_t *xm;                        // [rows, C] bf16
    int64_t rows, L, gate_bs, mod_bs;    // L rows per sequence; batch strides of the vectors in elements (0: one vector for all)
    int C, affine, round_xn;
    float eps;
};

// the launcher's row-length classes: a row of class NV has more than 512 * glue_sure(NV) columns, so its first glue_sure(NV) vectors lie
// wholly inside the row and need no bounds test
constexpr int glue_sure(int nv) { return nv == 3 ? 2 : nv == 6 ? 3 : nv == 10 ? 6 : nv == 16 ? 10 : 0; }

template <int NV, bool XBF, bool RES>   // NV 16-byte bf16 vectors per lane: 512 * glue_sure(NV) < C <= 512 * NV
__global__ __launch_bounds__(256) void residual_ln_modulate_f32_kernel(const GlueArgs a) {
    const int lane = threadIdx.x & 63, C = a.C;
    const int64_t wave = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const float inv_c = 1.0f / (float)C;
    const bool affine = a.affine != 0, round_xn = a.round_xn != 0;
    constexpr bool HELD = NV <= 6;
    constexpr int NH = HELD ? NV : 1, SURE = glue_sure(NV);
    f32x4 g[RES ? NH : 1][2], mu[NH][2], ad[NH][2];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f}, ones = {1.f, 1.f, 1.f, 1.f};
    // one vector j of the sequence's gate / multiplier / addend; columns past the row count as gate 1, multiplier 0, addend 0
    auto load_gate = [&](int64_t b, int j, f32x4 (&o)[2]) {
        const int c = (lane + 64 * j) * 8;
        o[0] = o[1] = ones;
        if (a.gate && (j < SURE || c < C)) {
            const float *p = a.gate + b * a.gate_bs + c;
            o[0] = *(const f32x4 *)p, o[1] = *(const f32x4 *)(p + 4);
        }
    };
    auto load_mod = [&](int64_t b, int j, f32x4 (&m)[2], f32x4 (&s)[2]) {
        const int c = (lane + 64 * j) * 8;
        m[0] = m[1] = s[0] = s[1] = zero;
        if (j < SURE || c < C) {
            const float *pm = a.mult + b * a.mod_bs + c, *ps = a.add + b * a.mod_bs + c;
            m[0] = *(const f32x4 *)pm, m[1] = *(const f32x4 *)(pm + 4), s[0] = *(const f32x4 *)ps, s[1] = *(const f32x4 *)(ps + 4);
            if (!affine) m[0] += 1.0f, m[1] += 1.0f;   // fp32(1 + scale), the tensor torch materialises
        }
    };
    int64_t held_b = -1;
    RowWalk w(wave, nwaves, a.L);
    for (int64_t r = wave; r < a.rows; r += nwaves, w.next()) {
        const int64_t b = w.b;
        if (HELD && b != held_b) {   // (wave-uniform: at most once per sequence the wave's rows reach)
            held_b = b;
#pragma unroll
            for (int j = 0; j < NH; ++j) {
                if constexpr (RES) load_gate(b, j, g[j]);
                load_mod(b, j, mu[j], ad[j]);
            }
        }
        float f[NV][8];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = (lane + 64 * j) * 8;
            const bool in = j < SURE || c < C;
            if constexpr (XBF) {
                u32x4 xv = {0u, 0u, 0u, 0u};
                if (in) xv = *(const u32x4 *)((const uint16_t *)a.x + r * C + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) f[j][2 * e] = __uint_as_float(xv[e] << 16), f[j][2 * e + 1] = __uint_as_float(xv[e] & 0xffff0000u);
            } else {
                f32x4 x0 = zero, x1 = zero;
                if (in) x0 = *(const f32x4 *)((const float *)a.x + r * C + c), x1 = *(const f32x4 *)((const float *)a.x + r * C + c + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) f[j][e] = x0[e], f[j][4 + e] = x1[e];
            }
            if constexpr (RES) {
                u32x4 yv = {0u, 0u, 0u, 0u};
                if (in) yv = *(const u32x4 *)(a.y + r * C + c);
                f32x4 gj[2];
                if constexpr (HELD) gj[0] = g[j][0], gj[1] = g[j][1];
                else load_gate(b, j, gj);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
#pragma clang fp contract(off)
                    const float yf = (e & 1) ? __uint_as_float(yv[e >> 1] & 0xffff0000u) : __uint_as_float(yv[e >> 1] << 16);
                    const float p = yf * gj[e >> 2][e & 3];   // rounded to fp32 (gate 1: y itself), then the sum: torch's two kernels
                    f[j][e] = f[j][e] + p;
                }
                if (in) {
                    float *dst = a.x_out + r * C + c;
                    *(f32x4 *)dst = (f32x4){f[j][0], f[j][1], f[j][2], f[j][3]};
                    *(f32x4 *)(dst + 4) = (f32x4){f[j][4], f[j][5], f[j][6], f[j][7]};
                }
            }
#pragma unroll
            for (int e = 0; e < 8; e += 2) sum += f[j][e] + f[j][e + 1];
        }
        const float mean = sum_across_rows(row16_sum(sum)) * inv_c;
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const bool in = j < SURE || (lane + 64 * j) * 8 < C;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                f[j][e] -= mean;
                ss = in ? __builtin_fmaf(f[j][e], f[j][e], ss) : ss;
            }
        }
        const float var = sum_across_rows(row16_sum(ss)) * inv_c;
        const float rstd = 1.0f / __builtin_sqrtf(var + a.eps);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = (lane + 64 * j) * 8;
            f32x4 m[2], s[2];
            if constexpr (HELD) m[0] = mu[j][0], m[1] = mu[j][1], s[0] = ad[j][0], s[1] = ad[j][1];
            else load_mod(b, j, m, s);
            u32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float p = f[j][2 * e] * rstd, q = f[j][2 * e + 1] * rstd;
                if (round_xn) round_bf16_pair(p, q);   // .type_as(x) of a bf16 x
                p = __builtin_fmaf(p, m[e >> 1][2 * (e & 1)], s[e >> 1][2 * (e & 1)]);
                q = __builtin_fmaf(q, m[e >> 1][2 * (e & 1) + 1], s[e >> 1][2 * (e & 1) + 1]);
                o[e] = pack_bf16x2(p, q);
            }
            if (j < SURE || c < C) *(u32x4 *)(a.xm + r * C + c) = o;
        }
    }
}

template <int NV>
void launch_glue(const GlueArgs &a, bool xbf, hipStream_t s) {
    // 4 rows per workgroup at a time; enough workgroups for 8 per CU, the rest of the rows by stride
    const int64_t want = (a.rows + 3) / 4;
    const dim3 grid((unsigned)(want < 256 * 8 ? want : 256 * 8)), block(256);
    if (a.y) {
        if (xbf) hipLaunchKernelGGL((residual_ln_modulate_f32_kernel<NV, true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((residual_ln_modulate_f32_kernel<NV, false, true>), grid, block, 0, s, a);
    } else {
        if (xbf) hipLaunchKernelGGL((residual_ln_modulate_f32_kernel<NV, true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((residual_ln_modulate_f32_kernel<NV, false, false>), grid, block, 0, s, a);
    }
}
}  // namespace

extern "C" int chipmunk_residual_ln_modulate_f32(const void *x, int x_dtype, const void *y, const float *gate, int64_t gate_batch_stride,
                                                 const float *shift, const float *scale, int64_t mod_batch_stride, const float *weight,
                                                 const float *bias, float *x_out, void *xm, int64_t B, int64_t L, int cols, double eps,
                                                 void *stream) {
    CM_CHECK(x && xm, "residual_ln_modulate_f32: null pointer");
    CM_CHECK(x_dtype == 1 || x_dtype == 2, "residual_ln_modulate_f32: x dtype code must be 1 (bf16) or 2 (fp32) (got %d)", x_dtype);
    CM_CHECK((y == nullptr) == (x_out == nullptr), "residual_ln_modulate_f32: y and x_out come together (both set: residual form; both null: LayerNorm only)");
    CM_CHECK(y || !gate, "residual_ln_modulate_f32: a gate without y");
    CM_CHECK(!(x_dtype == 1 && y && !gate), "residual_ln_modulate_f32: a bf16 x takes its residual with a gate (an ungated bf16 sum would stay bf16)");
    CM_CHECK((shift == nullptr) == (scale == nullptr) && (weight == nullptr) == (bias == nullptr),
             "residual_ln_modulate_f32: shift / scale come together, and so do weight / bias");
    CM_CHECK((shift != nullptr) != (weight != nullptr), "residual_ln_modulate_f32: exactly one of modulation (shift, scale) and affine (weight, bias)");
    CM_CHECK(cols > 0 && cols % 8 == 0 && cols <= 512 * 16, "residual_ln_modulate_f32: cols must be a multiple of 8, at most 8192 (got %d)", cols);
    CM_CHECK(B >= 1 && B < (1 << 24) && L >= 0 && L < ((int64_t)1 << 31), "residual_ln_modulate_f32: B must be in 1 .. 2^24 - 1 and L in 0 .. 2^31 - 1 (got B=%lld L=%lld)",
             (long long)B, (long long)L);
    CM_CHECK((gate_batch_stride == 0 || (gate && gate_batch_stride >= cols && gate_batch_stride % 4 == 0)) &&
                 (mod_batch_stride == 0 || (shift && mod_batch_stride >= cols && mod_batch_stride % 4 == 0)),
             "residual_ln_modulate_f32: a batch stride is 0 (one vector for every sequence) or a multiple of 4 elements that covers cols; weight / bias have none");
    CM_CHECK(((((uintptr_t)x | (uintptr_t)y | (uintptr_t)gate | (uintptr_t)shift | (uintptr_t)scale | (uintptr_t)weight | (uintptr_t)bias |
                (uintptr_t)x_out | (uintptr_t)xm)) & 15) == 0, "residual_ln_modulate_f32: pointers must be 16-byte aligned");
    if (L == 0) return CHIPMUNK_OK;
    GlueArgs a;
    a.x = x, a.y = (const uint16_t *)y, a.gate = gate;
    a.mult = shift ? scale : weight, a.add = shift ? shift : bias;
    a.x_out = x_out, a.xm = (uint16_t *)xm;
    a.rows = B * L, a.L = L, a.gate_bs = gate_batch_stride, a.mod_bs = mod_batch_stride;
    a.C = cols, a.affine = weight != nullptr, a.round_xn = x_dtype == 1 && !y && !weight;
    a.eps = (float)eps;
    hipStream_t s = (hipStream_t)stream;
    const int nv = (cols + 511) / 512;
    const bool xbf = x_dtype == 1;
    if (nv <= 2) launch_glue<2>(a, xbf, s);   // (the classes of glue_sure)
    else if (nv <= 3) launch_glue<3>(a, xbf, s);
    else if (nv <= 6) launch_glue<6>(a, xbf, s);
    else if (nv <= 10) launch_glue<10>(a, xbf, s);
    else launch_glue<16>(a, xbf, s);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}
