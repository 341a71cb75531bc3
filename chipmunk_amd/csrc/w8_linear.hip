// Weight-only fp8 linear layer for few rows (chipmunk_w8_linear; DESIGN 4.2, "Weight-only forward for few rows"):
//   y[M, F] = x[M, K] . f(w[F, K])^T, x bf16, w e4m3 (k-contiguous rows, as W8Linear.weight is stored), f the exact widening,
//   y[m, i] = bf16(bf16(S * scale_b[i]) + bias[i]), or bf16(S * scale_b[i]) without a bias; S the fp32 sum from zero over k.
// The kernel is bound by the weight stream, so the weight never touches LDS: for v_mfma_f32_16x16x32_bf16 the fragment of lane
// (n = lane % 16, kg = lane / 16) is 8 consecutive k of one weight row, and a lane loads 16 bytes of row i0 + n straight from global
// memory -- two fragments --, widened in registers (v_cvt_scalef32_pk_bf16_fp8 at scale 1.0, as mm1_w8_kernel does).  Within a 64-wide k
// step lane group kg therefore owns k = kg * 16 .. kg * 16 + 15: its first MFMA takes the lower 8, its second the upper 8, and the x
// fragments are read from LDS in that same order (16-byte chunk kg * 2 + h of the row's 128 bytes).
// A workgroup is 4 waves = 64 * NT output columns (16 * NT per wave) x one block of MT * 16 <= 128 rows; the accumulators stay in registers for
// all of K.  The weight tile is the MFMA's A operand and x its B operand, so a lane ends up with 4 consecutive output columns of one
// row: one 8-byte store.  x (small, L2-resident) is staged through LDS in whole 128-byte lines by plain loads + ds_write_b128, XOR-swizzled
// on the 16-byte chunk; weight and x loads of the next D k steps are in flight in registers (statically indexed: the k loop is unrolled
// by D), and since nothing is an LDS-DMA the one barrier per k step drains none of them.
// Row independence: output (m, i) is a chain of MFMAs over k = 0, 64, ... in which only row m of x and row i of w meet; neither the tile
// height MT, nor the prefetch depth, nor the other rows enter its bits.  K is never split.
#include "common.h"

#include <type_traits>

namespace {

struct W8LinParams {
    const uint16_t *x;
    const uint8_t *w;
    const float *scale_b;
    const uint16_t *bias;
    uint16_t *y;
    int64_t ldx, ldy;
    int M, K, F, scale_n;
};

template <int I>
using wic = std::integral_constant<int, I>;
template <int N, class Fn, int I = 0>
__device__ __forceinline__ void w8_static_for(Fn &&fn) {
    if constexpr (I < N) {
        fn(wic<I>{});
        w8_static_for<N, Fn, I + 1>(static_cast<Fn &&>(fn));
    }
}

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // scale_b is 4-byte aligned, no more

__device__ __forceinline__ f32x4 w8_scale(f32x4 a, f32x4 s) {
#pragma clang fp contract(off)
    return a * s;
}
__device__ __forceinline__ f32x4 w8_add(f32x4 a, f32x4 b) {
#pragma clang fp contract(off)
    return a + b;
}

// MT: 16-row tiles of the row block; NT: 16-column tiles of a wave (an x fragment read from LDS feeds NT MFMAs); D: k steps whose loads are in
// flight (even: the LDS buffer of a step is then a constant per slot)
template <int MT, int NT, int D>
__global__ __launch_bounds__(256) void w8_linear_kernel(const W8LinParams p) {
    static_assert(D % 2 == 0 && D >= 2, "two LDS buffers, addressed by the slot's parity");
    constexpr int RB = MT * 16;                // rows of the block
    constexpr int XB = RB * 128;               // bytes of one x stage: RB rows x 64 k
    constexpr int XI = (RB * 8 + 255) / 256;   // 16-byte chunks of a stage per thread
    __shared__ __attribute__((aligned(16))) unsigned char xs[2 * XB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ln = lane & 15, kg = lane >> 4;
    const int i0 = blockIdx.x * (64 * NT) + wave * (16 * NT);      // the wave's first output column
    const int row0 = blockIdx.y * RB;
    const int steps = p.K >> 6;

    // the lane's weight row (columns at and past F read row F - 1 and store nothing)
    const uint8_t *wp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wp[nt] = p.w + (size_t)min(i0 + nt * 16 + ln, p.F - 1) * p.K + kg * 16;

    // the thread's chunks of an x stage: chunk q = row q / 8, 16-byte piece q % 8; a row at or past M reads row M - 1 and is zeroed
    const uint16_t *xp[XI];
    int xl[XI];
    bool xv[XI];
#pragma unroll
    for (int i = 0; i < XI; ++i) {
        const int q = tid + 256 * i, r = (q >> 3) % RB, c = q & 7;
        xv[i] = row0 + r < p.M;
        xp[i] = p.x + (size_t)min(row0 + r, p.M - 1) * p.ldx + c * 8;
        xl[i] = r * 128 + ((c ^ ((r >> 1) & 7)) << 4);
    }

    u32x4 wr[D][NT], xr[D][XI];
    auto load = [&](int t, auto slot) {
        constexpr int S = decltype(slot)::value;
        const int tt = min(t, steps - 1);      // past the end: the last step again, never used
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wr[S][nt] = *(const u32x4 *)(wp[nt] + tt * 64);
#pragma unroll
        for (int i = 0; i < XI; ++i) xr[S][i] = *(const u32x4 *)(xp[i] + tt * 64);
    };
    auto stage = [&](auto slot) {              // x of the slot's step -> its LDS buffer
        constexpr int S = decltype(slot)::value;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const u32x4 v = xv[i] ? xr[S][i] : (u32x4){0u, 0u, 0u, 0u};
            if (RB * 8 % 256 == 0 || i + 1 < XI || tid + 256 * i < RB * 8) *(u32x4 *)(xs + (S & 1) * XB + xl[i]) = v;
        }
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    w8_static_for<D>([&](auto s) { load(decltype(s)::value, s); });
    stage(wic<0>{});
    __syncthreads();

    // one k step: the slot's weight fragments out of their registers, x of the next step into the other LDS buffer, the loads of step
    // t + D into the freed registers, then the MFMAs over this step's buffer; the barrier at the end orders both buffers
    auto step = [&](int t, auto slot) {
        constexpr int S = decltype(slot)::value;
        bf16x8 wf[NT][2];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u32x4 r = wr[S][nt];
            const bf16x2 f0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[2 * h], 1.0f, false), f1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[2 * h], 1.0f, true);
            const bf16x2 f2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[2 * h + 1], 1.0f, false), f3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[2 * h + 1], 1.0f, true);
            wf[nt][h] = (bf16x8){f0[0], f0[1], f1[0], f1[1], f2[0], f2[1], f3[0], f3[1]};
        }
        stage(wic<(S + 1) % D>{});
        load(t + D, slot);
        const unsigned char *xb = xs + (S & 1) * XB;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int rr = mt * 16 + ln;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bf16x8 xf = *(const bf16x8 *)(xb + rr * 128 + (((kg * 2 + h) ^ ((rr >> 1) & 7)) << 4));
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt][h], xf, acc[mt][nt], 0, 0, 0);
            }
        }
        __syncthreads();
    };
    int t = 0;
    for (; t + D <= steps; t += D) w8_static_for<D>([&](auto s) { step(t + decltype(s)::value, s); });
    w8_static_for<D - 1>([&](auto s) {
        if (t + decltype(s)::value < steps) step(t + decltype(s)::value, s);
    });

    // epilogue: per column tile the lane holds columns ic .. ic + 3 of row row0 + mt * 16 + ln (D[i][m]: i = (lane / 16) * 4 + j, m = lane % 16)
    const bool has_bias = p.bias != nullptr;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ic = i0 + nt * 16 + kg * 4;
        if (ic >= p.F) continue;               // F % 4 == 0: the four columns are in or out together
        f32x4 sv, bv = {0.f, 0.f, 0.f, 0.f};
        if (p.scale_n > 1) sv = *(const f32x4_a4 *)(p.scale_b + ic);
        else {
            const float s = p.scale_b[0];
            sv = (f32x4){s, s, s, s};
        }
        if (has_bias) {
            const u32x2 b = *(const u32x2 *)(p.bias + ic);
            bv = (f32x4){__uint_as_float(b[0] << 16), __uint_as_float(b[0] & 0xffff0000u), __uint_as_float(b[1] << 16), __uint_as_float(b[1] & 0xffff0000u)};
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = row0 + mt * 16 + ln;
            if (m >= p.M) continue;
            f32x4 v = w8_scale(acc[mt][nt], sv);
            if (has_bias) {
                v = (f32x4){hw_round_bf16(v[0]), hw_round_bf16(v[1]), hw_round_bf16(v[2]), hw_round_bf16(v[3])};
                v = w8_add(v, bv);
            }
            *(u32x2 *)(p.y + (size_t)m * p.ldy + ic) = (u32x2){pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        }
    }
}

template <int MT, int NT, int D>
int launch_w8_linear(const W8LinParams &p, hipStream_t s) {
    const dim3 grid((p.F + 64 * NT - 1) / (64 * NT), (p.M + MT * 16 - 1) / (MT * 16));
    hipLaunchKernelGGL((w8_linear_kernel<MT, NT, D>), grid, dim3(256), 0, s, p);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

}  // namespace

extern "C" int chipmunk_w8_linear(const void *x, int64_t ldx, const void *w, const float *scale_b, int scale_n, const void *bias, void *y,
                                  int64_t ldy, int M, int K, int F, void *stream) {
    CM_CHECK(x && w && scale_b && y, "w8_linear: null tensor or scale pointer");
    CM_CHECK(M >= 1 && K >= 64 && F >= 8, "w8_linear: M >= 1, K >= 64 and F >= 8 (got M = %d, K = %d, F = %d)", M, K, F);
    CM_CHECK(K % 64 == 0 && F % 8 == 0, "w8_linear: K must be a multiple of 64 and F a multiple of 8 (got K = %d, F = %d)", K, F);
    CM_CHECK(M <= CHIPMUNK_W8_LINEAR_MAX_M, "w8_linear: M = %d above the grid's %d rows", M, CHIPMUNK_W8_LINEAR_MAX_M);
    CM_CHECK(scale_n == 1 || scale_n == F, "w8_linear: scale_n must be 1 (one reciprocal scale) or F = %d (one per row of w), got %d", F, scale_n);
    CM_CHECK(((uintptr_t)scale_b & 3) == 0, "w8_linear: scale_b must be 4-byte aligned");
    CM_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)bias & 15) == 0 && ((uintptr_t)w & 15) == 0,
             "w8_linear: x, w, y and bias must be 16-byte aligned");
    CM_CHECK(ldx % 8 == 0 && ldy % 8 == 0, "w8_linear: ldx and ldy must be multiples of 8 elements (got %lld, %lld)", (long long)ldx, (long long)ldy);
    CM_CHECK(ldx >= K && ldy >= F, "w8_linear: ldx >= K and ldy >= F (got ldx = %lld, K = %d, ldy = %lld, F = %d)", (long long)ldx, K,
             (long long)ldy, F);
    const W8LinParams p = {(const uint16_t *)x, (const uint8_t *)w, scale_b, (const uint16_t *)bias, (uint16_t *)y, ldx, ldy, M, K, F, scale_n};
    hipStream_t s = (hipStream_t)stream;
    // the tile follows the row count (measured: docs/EXPERIMENTS_w8_linear.md); the bits of a row do not (see the head of this file)
    if (M <= 16) return launch_w8_linear<1, 1, 8>(p, s);
    if (M <= 32) return launch_w8_linear<2, 1, 8>(p, s);
    if (M <= 48) return launch_w8_linear<3, 1, 8>(p, s);
    if (M <= 64) return launch_w8_linear<4, 1, 8>(p, s);
    if (M <= 256) return launch_w8_linear<6, 1, 6>(p, s);      // 96-row blocks: more workgroups than 128-row ones, the x tile re-read less per wave
    return launch_w8_linear<8, 2, 4>(p, s);                    // many rows: 32 columns per wave, an x fragment feeds two MFMAs
}
