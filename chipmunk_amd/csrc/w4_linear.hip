// Weight-only MXFP4 linear layer for few rows (chipmunk_w4_linear; DESIGN 4.2, "MXFP4 forward for few rows"):
//   S[m, i] = sum over k of x[m, k] * wide(w)[i, k]      fp32, from zero; wide(w) = W4Linear.widened(), exact in bf16
//   y[m, i] = bf16(S[m, i] + float(bias[i]))             one rounding; without a bias bf16(S[m, i])
// x bf16 [M, K] (pitch ldx), w uint8 [F, K / 2] (element 2j of a row in bits 0 .. 3 of byte j), scale_b uint8 [F, K / 32] (e8m0, one byte per
// 32 k), bias bf16 [F] or null, y bf16 [M, F] (pitch ldy); K % 128 == 0, F % 8 == 0.  Scale byte 255 and widened values that are subnormal
// in bf16 are outside the contract (as for csp_mlp_mm1_w4).
// The kernel is bound by the weight stream (4.25 bits a weight), so the weight is read once from global memory and never touches LDS.  For
// v_mfma_f32_16x16x32_bf16 the fragment of lane (n = lane % 16, kg = lane / 16) is 8 consecutive k of one weight row = 4 bytes of nibbles; a
// lane loads 16 bytes of row i0 + n -- 32 k, exactly one e8m0 block, four fragments -- so the k step is 128: lane group kg owns
// k = 32 kg .. 32 kg + 31 of the step, its fragment h (bytes 4 h .. 4 h + 3) feeds the step's MFMA h, and the x fragments are read from LDS by
// the same permutation (16-byte chunk 4 kg + h of the row's 256 bytes).  A wave instruction touches 16 rows x 64 contiguous bytes.
// The block scale is applied at the conversion: v_cvt_scalef32_pk_bf16_fp4's scale operand is the e8m0 byte shifted into a float's exponent
// field (as mm1_tile's W4 form does), so the MFMA's A operand IS the widened bf16 weight and the epilogue has no scale.  The four scale
// bytes of a row and step are one aligned dword (K % 128 == 0); the four lane groups load the same dword and take byte kg by a shift.
// A workgroup is 4 waves = 64 * NT output columns (16 * NT per wave) x one block of MT * 16 <= 128 rows; the accumulators stay in registers for
// all of K, K is never split, there are no atomics.  The weight tile is the MFMA's A operand and x its B operand, so a lane ends with 4
// consecutive output columns of one row: one 8-byte store.  x (small, L2-resident) is staged through LDS in whole 256-byte lines by plain
// loads + ds_write_b128, two stages, one barrier per k step; chunk c of row r sits at chunk c ^ (r & 15): a row is one pass over the 64
// banks, the 16 lanes of a fragment read (rows r .. r + 15, one chunk index) land on 16 different chunks, and so do the 16 lanes that write
// one row (derived, not measured).  Weight, scale and x loads of the next D k steps are in flight in statically indexed registers (the k
// loop is unrolled by D); x keeps the depth of the weights because vmcnt counts in order: a shallower x ring would make the wait for an x
// line drain the weight loads issued before it.  Nothing is an LDS-DMA, so the barrier drains none of them.
// Row independence: output (m, i) is a chain of MFMAs over k = 0, 128, ... in which only row m of x and row i of w meet; neither the tile
// height MT, nor the prefetch depth, nor the other rows enter its bits.
#include "common.h"

#include <type_traits>

namespace {

struct W4LinParams {
    const uint16_t *x;
    const uint8_t *w;
    const uint8_t *scale_b;
    const uint16_t *bias;
    uint16_t *y;
    int64_t ldx, ldy;
    int M, K, F;
};

template <int I>
using w4ic = std::integral_constant<int, I>;
template <int N, class Fn, int I = 0>
__device__ __forceinline__ void w4_static_for(Fn &&fn) {
    if constexpr (I < N) {
        fn(w4ic<I>{});
        w4_static_for<N, Fn, I + 1>(static_cast<Fn &&>(fn));
    }
}

// (the HIP header's __uint_as_float is not force-inlined and would stay a call from a kernel compiled without the packed forms)
__device__ __forceinline__ float w4_bits_to_float(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ f32x4 w4_add(f32x4 a, f32x4 b) {
#pragma clang fp contract(off)
    return a + b;
}

// MT: 16-row tiles of the row block; NT: 16-column tiles of a wave (an x fragment read from LDS feeds NT MFMAs); D: k steps whose loads are in
// flight (even: the LDS buffer of a step is then a constant per slot).  Compiled without the packed fp32 VALU forms, as every new kernel of
// this library ("MXFP4 fc1"); the header's __syncthreads() would stay a call from such a kernel, so the barrier is written out.
template <int MT, int NT, int D>
__global__ __launch_bounds__(256) __attribute__((target("no-packed-fp32-ops"))) void w4_linear_kernel(const W4LinParams p) {
    static_assert(D % 2 == 0 && D >= 2, "two LDS buffers, addressed by the slot's parity");
    constexpr int RB = MT * 16;                // rows of the block
    constexpr int XB = RB * 256;               // bytes of one x stage: RB rows x 128 k
    constexpr int XI = MT;                     // 16-byte chunks of a stage per thread: RB * 16 / 256
    __shared__ __attribute__((aligned(16))) unsigned char xs[2 * XB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ln = lane & 15, kg = lane >> 4;
    const int i0 = blockIdx.x * (64 * NT) + wave * (16 * NT);      // the wave's first output column
    const int row0 = blockIdx.y * RB;
    const int steps = p.K >> 7;

    // the lane's weight row and its scale bytes (columns at and past F read row F - 1 and store nothing)
    const uint8_t *wp[NT];
    const uint8_t *sp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const size_t row = (size_t)min(i0 + nt * 16 + ln, p.F - 1);
        wp[nt] = p.w + row * (size_t)(p.K >> 1) + kg * 16;
        sp[nt] = p.scale_b + row * (size_t)(p.K >> 5);
    }

    // the thread's chunks of an x stage: chunk q = row q / 16, 16-byte piece q % 16; a row at or past M reads row M - 1 and is zeroed
    const uint16_t *xp[XI];
    int xl[XI];
    bool xv[XI];
#pragma unroll
    for (int i = 0; i < XI; ++i) {
        const int q = tid + 256 * i, r = q >> 4, c = q & 15;
        xv[i] = row0 + r < p.M;
        xp[i] = p.x + (size_t)min(row0 + r, p.M - 1) * p.ldx + c * 8;
        xl[i] = r * 256 + ((c ^ (r & 15)) << 4);
    }

    u32x4 wr[D][NT], xr[D][XI];
    uint32_t sr[D][NT];
    auto load = [&](int t, auto slot) __attribute__((always_inline)) {
        constexpr int S = decltype(slot)::value;
        const int tt = min(t, steps - 1);      // past the end: the last step again, never used
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            wr[S][nt] = *(const u32x4 *)(wp[nt] + tt * 64);
            sr[S][nt] = *(const uint32_t *)(sp[nt] + tt * 4);
        }
#pragma unroll
        for (int i = 0; i < XI; ++i) xr[S][i] = *(const u32x4 *)(xp[i] + tt * 128);
    };
    auto stage = [&](auto slot) __attribute__((always_inline)) {              // x of the slot's step -> its LDS buffer
        constexpr int S = decltype(slot)::value;
#pragma unroll
        for (int i = 0; i < XI; ++i) *(u32x4 *)(xs + (S & 1) * XB + xl[i]) = xv[i] ? xr[S][i] : (u32x4){0u, 0u, 0u, 0u};
    };
    auto barrier = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    w4_static_for<D>([&](auto s) __attribute__((always_inline)) { load(decltype(s)::value, s); });
    stage(w4ic<0>{});
    barrier();

    // one k step: the slot's four weight fragments out of their registers (the block's scale at the conversion), x of the next step into the
    // other LDS buffer, the loads of step t + D into the freed registers, then the MFMAs over this step's buffer; the barrier at the end
    // orders both buffers
    auto step = [&](int t, auto slot) __attribute__((always_inline)) {
        constexpr int S = decltype(slot)::value;
        bf16x8 wf[NT][4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const u32x4 r = wr[S][nt];
            const float sc = w4_bits_to_float(((sr[S][nt] >> (kg * 8)) & 0xffu) << 23);   // 2^(s - 127): the e8m0 byte is the exponent field
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const bf16x2 f0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(r[h], sc, 0), f1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(r[h], sc, 1);
                const bf16x2 f2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(r[h], sc, 2), f3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(r[h], sc, 3);
                wf[nt][h] = (bf16x8){f0[0], f0[1], f1[0], f1[1], f2[0], f2[1], f3[0], f3[1]};
            }
        }
        stage(w4ic<(S + 1) % D>{});
        load(t + D, slot);
        const unsigned char *xb = xs + (S & 1) * XB;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int rr = mt * 16 + ln;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const bf16x8 xf = *(const bf16x8 *)(xb + rr * 256 + (((kg * 4 + h) ^ ln) << 4));   // rr & 15 == ln
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt][h], xf, acc[mt][nt], 0, 0, 0);
            }
        }
        barrier();
    };
    int t = 0;
    for (; t + D <= steps; t += D) w4_static_for<D>([&](auto s) __attribute__((always_inline)) { step(t + decltype(s)::value, s); });
    w4_static_for<D - 1>([&](auto s) __attribute__((always_inline)) {
        if (t + decltype(s)::value < steps) step(t + decltype(s)::value, s);
    });

    // epilogue: per column tile the lane holds columns ic .. ic + 3 of row row0 + mt * 16 + ln (D[i][m]: i = (lane / 16) * 4 + j, m = lane % 16)
    const bool has_bias = p.bias != nullptr;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ic = i0 + nt * 16 + kg * 4;
        if (ic >= p.F) continue;               // F % 4 == 0: the four columns are in or out together
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (has_bias) {
            const u32x2 b = *(const u32x2 *)(p.bias + ic);
            bv = (f32x4){w4_bits_to_float(b[0] << 16), w4_bits_to_float(b[0] & 0xffff0000u), w4_bits_to_float(b[1] << 16), w4_bits_to_float(b[1] & 0xffff0000u)};
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = row0 + mt * 16 + ln;
            if (m >= p.M) continue;
            const f32x4 v = has_bias ? w4_add(acc[mt][nt], bv) : acc[mt][nt];
            *(u32x2 *)(p.y + (size_t)m * p.ldy + ic) = (u32x2){pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        }
    }
}

template <int MT, int NT, int D>
int launch_w4_linear(const W4LinParams &p, hipStream_t s) {
    const dim3 grid((p.F + 64 * NT - 1) / (64 * NT), (p.M + MT * 16 - 1) / (MT * 16));
    hipLaunchKernelGGL((w4_linear_kernel<MT, NT, D>), grid, dim3(256), 0, s, p);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

}  // namespace

extern "C" int chipmunk_w4_linear(const void *x, int64_t ldx, const void *w, const uint8_t *scale_b, const void *bias, void *y, int64_t ldy,
                                  int M, int K, int F, void *stream) {
    CM_CHECK(x && w && scale_b && y, "w4_linear: null x, w, scale_b or y");
    CM_CHECK(M >= 1 && K >= 128 && F >= 8, "w4_linear: M >= 1, K >= 128 and F >= 8 (got M = %d, K = %d, F = %d)", M, K, F);
    CM_CHECK(K % 128 == 0 && F % 8 == 0, "w4_linear: K must be a multiple of 128 and F a multiple of 8 (got K = %d, F = %d)", K, F);
    CM_CHECK(M <= CHIPMUNK_W4_LINEAR_MAX_M, "w4_linear: M = %d above the grid's %d rows", M, CHIPMUNK_W4_LINEAR_MAX_M);
    CM_CHECK(((uintptr_t)scale_b & 3) == 0, "w4_linear: scale_b must be 4-byte aligned");
    CM_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)bias & 15) == 0 && ((uintptr_t)w & 15) == 0,
             "w4_linear: x, w, y and bias must be 16-byte aligned");
    CM_CHECK(ldx % 8 == 0 && ldy % 8 == 0, "w4_linear: ldx and ldy must be multiples of 8 elements (got %lld, %lld)", (long long)ldx, (long long)ldy);
    CM_CHECK(ldx >= K && ldy >= F, "w4_linear: ldx >= K and ldy >= F (got ldx = %lld, K = %d, ldy = %lld, F = %d)", (long long)ldx, K,
             (long long)ldy, F);
    const W4LinParams p = {(const uint16_t *)x, (const uint8_t *)w, scale_b, (const uint16_t *)bias, (uint16_t *)y, ldx, ldy, M, K, F};
    hipStream_t s = (hipStream_t)stream;
    // the tile follows the row count (docs/EXPERIMENTS_w4_linear.md); the bits of a row do not (see the head of this file)
    if (M <= 16) return launch_w4_linear<1, 1, 8>(p, s);
    if (M <= 32) return launch_w4_linear<2, 1, 8>(p, s);
    if (M <= 48) return launch_w4_linear<3, 1, 8>(p, s);
    if (M <= 64) return launch_w4_linear<4, 1, 8>(p, s);
    if (M <= 256) return launch_w4_linear<6, 1, 4>(p, s);      // 96-row blocks, 48 KiB of LDS: three workgroups a CU
    return launch_w4_linear<8, 2, 2>(p, s);                    // many rows: 32 columns per wave, an x fragment feeds two MFMAs; 64 KiB of LDS
}
