// Column-sparse ("delta") MLP GEMMs for gfx950.
// Replaces reference csrc/mlp/csp_mlp_mm1.cu, csrc/mlp/csp_mlp_mm2_and_scatter_add.cu (+ the Triton GEMM
// src/chipmunk/triton/csp_mlp_mm2.py) and csrc/indexed_io/scatter_add.cu.
//
// Both GEMMs: workgroup tile = 128 rows (one sparsity group, reference bm = 128) x BN packed columns, K step BK, 4 or 8
// waves, v_mfma_f32_32x32x16_bf16 accumulators, NST-deep LDS ring filled by buffer-form LDS-DMA
// (buffer_load_dwordx4 ... lds) with counted vmcnt across a raw s_barrier; shapes are template parameters, the shipped
// ones are GEMM1 <128 cols, K step 64, 2 stages, 2 workgroups/CU, 4 waves of 64x64> and GEMM2 <256, 32, 3, 2, 8 waves
// of 64x64>.  The gather is the per-lane source offset of the DMA: fc1 rows (mm1) are 2*K contiguous bytes, fc2^T rows
// (mm2) are 2*N2 contiguous bytes, so every gathered piece is a full 128-byte line.  XOR swizzles are applied on the
// source chunk index so the lane-linear LDS image is conflict-free for ds_read_b128 (k-contiguous operands) and
// ds_read_b64_tr_b16 (fc2^T, which is n-contiguous in memory and must be fed k-contiguous to the MFMA).  Epilogues go
// through the freed ring so that global memory only sees 16-byte accesses over whole row segments.
// GEMM2 also exists over e4m3 rows of fc2^T (mm2_w8_kernel, weight-only fp8): the gathered row slice is N2 BYTES, the transpose read runs over
// the byte image with a column pair as its 16-bit element, v_perm_b32 + v_cvt_scalef32_pk_bf16_fp8 widen to bf16 in registers in front of the
// same bf16 MFMA, and the freed half of the B tile is a fourth ring stage <256, 32, 4, 2, 8 waves>.
// GEMM1 has the same weight-only form over e4m3 rows of fc1 (mm1_w8_kernel, mm1_tile's W8): the gathered piece of a k step is 64 BYTES, k-contiguous,
// so a fragment is one ds_read_b64 widened by v_cvt_scalef32_pk_bf16_fp8, no transpose; three stages of 16 + 8 KiB under the FLAT epilogue.
#include "common.h"
#include "attn64_util.h"
#include <type_traits>

namespace {

constexpr int BM = 128;  // rows per workgroup = one sparsity group (reference bm = 128)

#ifdef MLP_PROF
// Cycle anatomy of the GEMM k loops (tools/mlp_prof.py builds a separate library with -DMLP_PROF): s_memtime at the segment
// boundaries of every k step, per wave of one mid-grid workgroup.  Not part of the product build.
__device__ unsigned long long g_mlp_prof[16 * 8];
#define MPROF_DECL unsigned long long pt_ = 0, pacc_[6] = {0, 0, 0, 0, 0, 0}; const bool prof_on_ = blockIdx.x == 161
#define MPROF_START() do { if (prof_on_) pt_ = __builtin_amdgcn_s_memtime(); } while (0)
#define MPROF_MARK(i) do { if (prof_on_) { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); pacc_[i] += n_ - pt_; pt_ = n_; } } while (0)
#define MPROF_ABS(i) do { if (blockIdx.x == 161 && (threadIdx.x & 63) == 0) g_mlp_prof[96 + (threadIdx.x >> 6) * 4 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#define MPROF_END(w, n) do { if (prof_on_ && (threadIdx.x & 63) == 0) { for (int i_ = 0; i_ < 6; ++i_) g_mlp_prof[(w) * 8 + i_] = pacc_[i_]; g_mlp_prof[(w) * 8 + 7] = (n); } } while (0)
extern "C" int chipmunk_mlp_prof_read(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mlp_prof), sizeof(g_mlp_prof)) == hipSuccess ? 0 : 2;
}
#else
#define MPROF_DECL
#define MPROF_START()
#define MPROF_MARK(i)
#define MPROF_END(w, n)
#define MPROF_ABS(i)
#endif


__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// tanh-GeLU (reference csrc/common/elementwise/gelu.cuh:26-30): x*0.5*(1+tanh(u)) == x*(1 - 1/(1+exp(2u))), u = 0.79788456*(x + 0.044715 x^3);
// evaluated as x - x / (1 + exp2(x * (GA + GB x^2))).  The 2-wide form is the same operation sequence on v_pk_*_f32 (the epilogue
// is VALU-bound: tools/mlp_prof.py, 18 k of a tile's 103 k cycles before this form), element-for-element the same bits.
constexpr float GELU_A = 0.7978845608028654f * 2.0f * 1.44269504089f, GELU_B = GELU_A * 0.044715f;
__device__ __forceinline__ uint32_t pack_bf16x2_v(f32x2 v) { return pack_bf16x2(v[0], v[1]); }   // v_cvt_pk_bf16_f32, RNE
__device__ __forceinline__ f32x2 unpack_bf16x2(uint32_t u) { return (f32x2){__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)}; }
__device__ __forceinline__ float gelu_tanh(float x) {
    const float t = __builtin_fmaf(x * x, GELU_B, GELU_A);
    const float e = __builtin_amdgcn_exp2f(x * t);
    return __builtin_fmaf(-x, __builtin_amdgcn_rcpf(e + 1.0f), x);
}
__device__ __forceinline__ f32x2 gelu_tanh2(f32x2 x) {
    const f32x2 t = __builtin_elementwise_fma(x * x, (f32x2){GELU_B, GELU_B}, (f32x2){GELU_A, GELU_A});
    const f32x2 u = x * t;
    const f32x2 d = (f32x2){__builtin_amdgcn_exp2f(u[0]), __builtin_amdgcn_exp2f(u[1])} + (f32x2){1.0f, 1.0f};
    const f32x2 r = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    return __builtin_elementwise_fma(-x, r, x);
}

// Activations of the gated GEMM1 (CHIPMUNK_ACT_*): 0 is the tanh-GeLU above, the same code; 1 SiLU x / (1 + exp(-x)); 2 the exact GeLU
// 0.5 x (1 + erf(x / sqrt 2)).
template <int ACT>
__device__ __forceinline__ f32x2 glu_act2(f32x2 x) {
    static_assert(ACT >= 0 && ACT <= 2, "unknown activation");
    if constexpr (ACT == 0) {
        return gelu_tanh2(x);
    } else if constexpr (ACT == 1) {
        const f32x2 u = x * (f32x2){-1.44269504089f, -1.44269504089f};
        const f32x2 d = (f32x2){__builtin_amdgcn_exp2f(u[0]), __builtin_amdgcn_exp2f(u[1])} + (f32x2){1.0f, 1.0f};
        return x * (f32x2){__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    } else {
        const f32x2 e = {erff(x[0] * 0.70710678118654752f), erff(x[1] * 0.70710678118654752f)};
        return (x * (f32x2){0.5f, 0.5f}) * (e + (f32x2){1.0f, 1.0f});
    }
}

// (scalar twin, for the direct epilogue of the ungated GEMM1: the same operation sequence per element)
template <int ACT>
__device__ __forceinline__ float glu_act(float x) {
    static_assert(ACT >= 0 && ACT <= 2, "unknown activation");
    if constexpr (ACT == 0) return gelu_tanh(x);
    else if constexpr (ACT == 1) return x * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(x * -1.44269504089f) + 1.0f);
    else return (x * 0.5f) * (erff(x * 0.70710678118654752f) + 1.0f);
}

// a * s + b as a multiplication and an addition, each rounded: never contracted into an fma
__device__ __forceinline__ f32x2 scale_then_bias2(f32x2 a, f32x2 s, f32x2 b) {
#pragma clang fp contract(off)
    const f32x2 t = a * s;
    return t + b;
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt immediate out of range");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Geometry of a k-contiguous operand tile [ROWS][BK] bf16 staged by LDS-DMA:
//   row stride BK*2 bytes, CPR = BK/8 16-byte chunks per row, one DMA instruction (64 lanes x 16 B) covers RPI rows;
//   chunk c of row r is stored at chunk c ^ swz(r), swz(r) = (r / RPB) & (CPR-1), RPB = rows per 256-byte bank row:
//   conflict-free for the ds_read_b128 lane groups of a 32-row MFMA operand fragment.
template <int BK>
struct KTile {
    static constexpr int ROWB = BK * 2, CPR = BK / 8, RPI = 1024 / ROWB, RPB = 256 / ROWB;
    __device__ static __forceinline__ int swz(int row) { return (row / RPB) & (CPR - 1); }
    // source element offset inside a row for the lane's stored chunk
    __device__ static __forceinline__ int src_chunk_elems(int row, int lane) { return ((lane % CPR) ^ swz(row)) << 3; }
    __device__ static __forceinline__ int lane_row(int inst, int lane) { return inst * RPI + lane / CPR; }
    __device__ static __forceinline__ bf16x8 frag(const unsigned char *tile, int row, int kk, int lane) {
        const int c = kk * 2 + (lane >> 5);
        return *(const bf16x8 *)(tile + row * ROWB + ((c ^ swz(row)) << 4));
    }
};


// Live-tile map shared by both GEMMs.  The host launches G x NTmax workgroups without knowing the per-group counts
// (they live in HBM); every workgroup derives the same compact order from them:
//   * only column tiles below max_g counts[g] are live (a dead workgroup exits in a few hundred cycles);
//   * the live tiles are split into 8 contiguous chunks, one per XCD (block b runs on XCD b % 8);
//   * inside a chunk consecutive tiles walk "NR column tiles x all groups": with ascending index lists the tiles of
//     DIFFERENT groups over the same column-tile position gather overlapping weight rows, so the ~64 workgroups an XCD
//     runs at once re-use each other's rows (and each group's activation tile) out of that XCD's 4 MiB L2 instead of
//     re-fetching them through the fabric.  Measured on FLUX shapes: fabric fetch per launch 860 MB -> see DESIGN.md.
//   * tail split (NSUB > 1): workgroups are dispatched in block order as slots free up, so with T equal tiles on S
//     resident slots the last T mod S tiles run alone for a whole tile time (FLUX: 34 groups x 32 column tiles = 1088
//     tiles on 512 slots -> the third "round" is 12 % full and costs a third of the launch).  When an XCD's leftover
//     is small, each leftover tile is handed out as NSUB quarter-size sub-tiles (64 x 64 outputs, full K, deeper
//     ring) to NSUB workgroups at the END of that XCD's block range.  Every output element is still produced by one
//     workgroup with the same K order, so results are bit-identical to the unsplit schedule.
struct TileMap {
    int g, nt, sub;  // sub < 0: whole tile
    bool live;
};
// The part of the map that is the same for every tile of a workgroup: live column tiles, this XCD's share and where its tail begins.
struct TilePlan {
    int G, NR, NTl, mine, full, base, nsub;
    // workgroup slots of this XCD that carry work: whole tiles, then the tail's sub-tiles
    __device__ __forceinline__ int slots() const { return full + (mine - full) * nsub; }
};
template <int BN>
__device__ __forceinline__ TilePlan plan_tiles(const int32_t *counts, int G, int NTmax, int NR, int slots_per_xcd = 0, int nsub = 1) {
    int cmax = 0;  // wave-parallel max (a scalar loop over G costs ~50 ns per group, per workgroup)
    for (int g = threadIdx.x & 63; g < G; g += 64) cmax = max(cmax, counts[g]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cmax = max(cmax, __shfl_xor(cmax, off));
    cmax = __builtin_amdgcn_readfirstlane(cmax);
    TilePlan pl;
    pl.G = G, pl.NR = NR, pl.nsub = nsub;
    pl.NTl = min((cmax + BN - 1) / BN, NTmax);
    const int total = pl.NTl * G;
    const int xcd = blockIdx.x & 7;
    const int q = total >> 3, r = total & 7;
    pl.mine = q + (xcd < r ? 1 : 0);  // tiles of this XCD
    pl.full = pl.mine;
    if (nsub > 1 && slots_per_xcd > 0) {
        const int rem = pl.mine % slots_per_xcd;
        if (pl.mine > slots_per_xcd && rem > 0 && rem * nsub <= slots_per_xcd) pl.full = pl.mine - rem;
    }
    pl.base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return pl;
}
__device__ __forceinline__ TileMap tile_at(const TilePlan &pl, int slot) {
    TileMap m;
    m.sub = -1;
    if (slot >= pl.full) {
        const int k = slot - pl.full;
        m.sub = k % pl.nsub;
        slot = pl.full + k / pl.nsub;
    }
    m.live = slot < pl.mine;
    const int t = pl.base + slot;
    const int per = pl.G * pl.NR;
    const int nb = t / per, rem = t - nb * per;
    const int nr = min(pl.NR, pl.NTl - nb * pl.NR);
    m.g = nr > 0 ? rem / nr : 0;
    m.nt = nb * pl.NR + (nr > 0 ? rem - m.g * nr : 0);
    return m;
}

// ------------------------------------------------------------------------------------------------ mm1
struct Mm1Params {
    const uint16_t *a, *b, *bias;
    uint16_t *cache;
    uint16_t *c;
    const int32_t *indices, *counts;
    int M, K, F, NT, NR, probe, slots_per_xcd;
    int update_cache;  // 1: also apply the scatter-add of this tile's deltas to the cache block it already holds in LDS;
                       // 2 (fp8): store the new activation into the cache like the reference's Triton kernel
    // fp8 only: reciprocal quantisation scales (one float each).  The gated form (GLU; its bf16 form has no scales, its fp8 form its own block below) keeps the up
    // projection's weight and bias in the same two slots -- b / bias are then the gate projection's, either bias may be null (= zero):
    // the parameter block keeps its size, and with it every kernel-argument offset of the ungated instantiations
    union { const float *scale_a; const uint16_t *b_up; };
    union { const float *scale_b; const uint16_t *bias_up; };
    int ldc;           // pitch of the column-major cache in elements: ldc >= M, ldc % 8 == 0 (M itself for the [F, M] contiguous cache)
    // elements between the row groups of one column: element (column i, row g * BM + r) of the cache is cache[i * ldc + g * gs + r].
    // BM: the column-major cache [F, ldc].  F * BM with ldc = BM: the group-major cache [G, F, BM] (the *_gm entries), whose 256-byte
    // pieces of one group lie on a 256-byte grid inside one F * 256-byte window.  (The field fills the block's tail padding: no size change.)
    int gs = BM;
};
// The gated fp8 form needs both at once -- the up projection's weight / bias AND scales -- so it has a parameter block of its own behind the
// shared one (which keeps its size): b / bias / b_up / bias_up as in the gated bf16 form (weights e4m3 bytes), then the three reciprocal
// quantisation scales, one float each.  mm1_tile takes its parameter block as a template type and reads these only in its FP8 && GLU form.
struct Mm1GluF8Params : Mm1Params {
    const float *scale_x, *scale_gate, *scale_up;
};
// The weight-only form (mm1_w8_kernel): b is the e4m3 weight [F, K], scale_b its reciprocal scale -- one number (scale_n == 1) or one per
// fc1 row (scale_n == F); which, is this run-time field behind the shared block.  scale_a is not read.
struct Mm1W8Params : Mm1Params {
    int scale_n;
};
// The gated weight-only form (mm1_glu_w8_kernel): b / b_up are the e4m3 gate / up weights [F, K] (b_up / bias_up in the union slots as in the
// gated bf16 form: the shared block keeps its size), each with a reciprocal scale of its own -- one number (_n == 1) or one per row (_n == F).
struct Mm1GluW8Params : Mm1Params {
    const float *scale_gate, *scale_up;
    int scale_gate_n, scale_up_n;
};

// One TM x TN output tile (TM rows of group g starting at m_off, packed columns n0 .. n0+TN-1): 4 waves as 2 x 2, each a
// (TM/2) x (TN/2) accumulator of 32x32x16 MFMA tiles; NST-deep LDS ring of [A tile | B tile] stages.
// FP8: operands are OCP e4m3 bytes (BASELINE config C5; reference src/chipmunk/triton/csp_mlp_mm1.py:37-164); BK then
// still counts 2-byte units, i.e. a k step is BK*2 = 128 bytes of every row either way.
// NW = 8 (round 4, option mm1_variant = 10; NOT the default): the same 64 x 64 accumulator per wave, 2 x 4 waves over a 128 x 256 tile -- two
// waves per SIMD out of ONE workgroup per CU instead of two 128 x 128 workgroups: 48 KiB instead of 64 KiB through the L2 -> LDS path per
// 128 x 256 outputs and k step, three stages in 144 KiB.  MEASURED SLOWER: 145-149 vs 117-125 us (FLUX bf16), 231-234 vs 206-222 us
// (Wan fp8), tools/mlp_prof.py: 2 000 ticks per k step against 1 620 for the PAIR of 128 x 128 workgroups, and an epilogue of 12.8 k
// ticks that nothing overlaps (two independent workgroups run one's epilogue under the other's k loop; here all eight waves sit in it).
// Neither the second wave of a SIMD issuing its DMA pieces after its MFMAs (2 200 per step) nor the pieces spread between the MFMA
// groups (no change; the 4-wave form 125 -> 131 us bf16, 219 -> 212 us fp8, inside box noise) helps: the loop waits on the
// landing of the gathered rows, not on their bytes or their issue.
// GLU (gated feed-forward, c = bf16(act(x Wg + bg) * (x Wu + bu) - cache)): the B tile keeps its TN rows but holds TN/2 packed columns x
// {gate, up}.  A wave's 64-row slab is split by n4: n4 = 0 holds the gate rows of packed columns n0 + wn*32 + (lane&31), n4 = 1 the up rows of
// the same 32 columns, so a lane holds acc[mt][0][r] (gate) and acc[mt][1][r] (up) of one (row, column) and the epilogue combines them
// without cross-lane traffic, on today's accumulator budget.  One DMA instruction covers KTile::RPI consecutive tile rows, so the half
// (and with it the weight the rows are gathered from) is uniform per instruction.  Cache block and output image are TN/2 columns wide.
// FP8 && GLU (P = Mm1GluF8Params): the k loop of the fp8 form (e4m3 fragments, 32x32x64 MFMA, accumulators from zero) under the B-row gather
// and the epilogue of the gated form; each branch's sum is scaled by scale_x and its own weight scale, then biased, in the fp8 form's order.
// Ungated forms with ACT != 0 or NULLB (mm1_form_kernel): c = bf16(act(x W + b) - cache) with act one of CHIPMUNK_ACT_*, and a null bias vector
// read as zero -- bf16 seeds its accumulators with 0, fp8 adds 0 behind the scales.  ACT = 0 without NULLB is the code mm1_kernel always had.
// RS (ungated fp8 only; chipmunk_csp_mlp_mm1_fp8_act_rs): scale_a is a vector over the token rows ([M]), scale_b one over the fc1 columns ([F]).
// The column's scale is a per-lane scalar like its bias -- gathered through the indices in the prologue --, the row scales of a lane's runs of
// four rows are fetched behind the k loop, under the wait for the cache block: the loop carries nothing new.  Rows at or past M read a live
// row's scale (as their A rows do) and are never stored.  (acc * scale_a[m]) * scale_b[i] + bias[i]: the scalar form's order and its bits.
// W8 (mm1_w8_kernel; P = Mm1W8Params): bf16 a, e4m3 weight rows, weight-only.  The A tile and its fragments are the bf16 form's; a B row piece
// of one k step is BK BYTES, so the B tile has KTile<BK / 2>'s shape (64-byte rows, 16 per DMA instruction).  A lane's fragment of MFMA slice kk
// is the 8 bytes at byte (kk * 2 + (lane >> 5)) * 8 of its row -- half (lane >> 5) of 16-byte chunk kk --, one ds_read_b64, widened to bf16x8 by
// v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 (exact) in front of the bf16 MFMA: k sits where the bf16 form puts it, so the fp32 sums are the bf16
// form's on the widened weight.  Banks: the 32 lanes of a ds_read_b64 group share their chunk HALF, so on a 16-byte grid they can reach only 32 of
// the 64 banks whatever the chunk swizzle does; the swizzle (chunk c of row r at chunk c ^ (r / 4 & 3): 16 rows x 4 chunks -> the 16 chunk positions
// of a 256-byte bank row) is therefore completed by a shift of every odd 1-KiB DMA piece by 8 bytes -- rows 0 .. 15 of a 32-row fragment read the
// dword pairs {4p, 4p + 1}, rows 16 .. 31 the pairs {4p + 2, 4p + 3} (+ 2 for the upper lane half): 64 banks, once each.  A shifted piece
// ends 8 bytes behind its KiB, so every PAIR of pieces (one 32-row fragment) owns 2 KiB + 16 bytes: an even piece at the pair's start, the odd
// one 1 KiB + 8 behind it (a pair's start moves all its 32 rows by the same number of banks).  The sum starts from zero, is multiplied by the gathered column's reciprocal scale (p.scale_n == 1:
// one number for all) and then biased, two roundings, never an fma; act and the subtraction are the bf16 form's, one rounding.
// GLU && W8 (mm1_glu_w8_kernel; P = Mm1GluW8Params): the two composed.  The B tile is W8's: TN = 128 rows of BK = 64 bytes, KTile<32>, 16 rows per
// DMA instruction, so instruction I of the tile's 8 covers tile rows [16 I, 16 I + 16) and wave w issues I = 2 w and 2 w + 1 -- the even and the
// odd piece of PAIR w, tile rows [32 w, 32 w + 32).  The gated form assigns tile rows [64 wn + 32 half, +32) to the gate (half 0) or the up (half 1)
// rows of packed columns n0 + 32 wn + (lane & 31); a pair's 32 rows start at a multiple of 32, so they lie inside one such range: pair w holds
// half w & 1 of wave column wn = w >> 1, whole.  Both pieces of a pair therefore gather from ONE weight, (16 I >> 5) & 1 = w & 1 is wave-uniform
// per instruction (here: per wave), and nothing of the LDS image moves: the row a lane reads for (wn, n4) is 64 wn + 32 n4 + (lane & 31) in the
// gated and in the ungated form alike, pair (row >> 5), piece (row >> 4) & 1, so swizzle, 8-byte shift and the bank argument above hold
// unchanged -- only the SOURCE of rows 32 .. 63 and 96 .. 127 differs.  k loop: W8's (sums from zero, k where the bf16 gated form puts it).
// Epilogue: g = (sum_g * scale_gate[i]) + bias_gate[i], u = (sum_u * scale_up[i]) + bias_up[i], each a rounded multiply and a rounded add
// (scale_then_bias2), then the gated form's fma(act(g), u, -cache), one rounding.  EPI = TM * 64 * 2 = 16 KiB fits a 24 640-byte stage: the plain
// staged epilogue, cache block and output image in one stage each.
template <int TM, int TN, int BK, int NST, bool FP8 = false, int NW = 4, bool GLU = false, int ACT = 0, class P = Mm1Params, bool NULLB = false,
          bool RS = false, bool W8 = false>
__device__ __forceinline__ void mm1_tile(const P &p, unsigned char *smem, int g, int m_off, int n0, int cnt) {
    static_assert(!RS || (FP8 && !GLU && NULLB), "row / column scale vectors: the ungated fp8 form with a nullable bias (mm1_form_kernel) only");
    static_assert(!W8 || (!FP8 && !RS && (GLU || NULLB) && NW == 4 && BK == 64), "the weight-only form: bf16 a, 4 waves, 64-byte B row pieces");
    static_assert(!(W8 && GLU) || std::is_base_of<Mm1GluW8Params, P>::value, "the gated weight-only form reads its scales from Mm1GluW8Params");
    using KT = KTile<BK>;
    using KTB = KTile<W8 ? BK / 2 : BK>;     // the B tile's geometry
    constexpr uint32_t ESZ = FP8 ? 1u : 2u;  // operand element size in bytes
    constexpr uint32_t BSZ = W8 ? 1u : ESZ;  // ... of the weight
    constexpr int B_PAD = W8 ? TN / 32 * 16 : 0;   // (W8: 16 bytes per pair of DMA pieces, room for the odd piece's 8-byte shift)
    constexpr int B_PAIR = 2048 + 16;              // (W8: bytes a pair of pieces owns)
    constexpr int A_TILE = TM * BK * 2, B_TILE = TN * BK * (int)(W8 ? 1 : 2) + B_PAD, STAGE = A_TILE + B_TILE;
    constexpr int A_INST = A_TILE / (1024 * NW), B_INST = (B_TILE - B_PAD) / (1024 * NW);  // DMA instructions per wave per tile
    constexpr int WNC = NW / 2;                                     // waves across the tile's columns (2 down its rows)
    constexpr int MT = TM / 64, NT4 = TN / (32 * WNC);              // 32-wide m / n tiles per wave
    static_assert(A_INST >= 1 && B_INST >= 1, "tile too small for one DMA instruction per wave");
    constexpr int PW = GLU ? TN / 2 : TN;                           // packed columns of the tile
    constexpr int NP4 = GLU ? 1 : NT4;                              // 32-wide tiles of packed columns per wave
    static_assert(!GLU || (NW == 4 && NT4 == 2 && 32 % KTB::RPI == 0), "the gated form: 4 waves, a 64-row B slab per wave");
    static_assert(!(FP8 && GLU) || std::is_base_of<Mm1GluF8Params, P>::value, "the gated fp8 form reads its scales from Mm1GluF8Params");
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w / WNC, wn = w % WNC;
    const int32_t *idxg = p.indices + (int64_t)g * p.F;

    // Ragged last group (M % 128 != 0): `rows` of the tile's TM rows exist.  An A row only feeds its own output row, so the LDS rows
    // past `rows` may hold anything as long as they are never stored: their DMA pieces re-read the tile's last live row (as the B rows
    // past the count re-read a live one), and the epilogue masks its stores by row.  The descriptors of a and the cache carry the real
    // sizes, so an offset past the tensor would be dropped by the range check, not fetched.
    const int rows = min(TM, p.M - (g * BM + m_off));
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(p.a, (uint32_t)p.M * p.K * ESZ), rb = make_rsrc(p.b);
    const __amdgpu_buffer_rsrc_t rb_up = make_rsrc(GLU ? p.b_up : p.b);   // (gated form: the weight the up rows are gathered from)
    uint32_t aoff[A_INST], boff[B_INST];  // byte offsets
#pragma unroll
    for (int i = 0; i < A_INST; ++i) {
        const int row = KT::lane_row(w * A_INST + i, lane);
        aoff[i] = (uint32_t)(g * BM + m_off + min(row, rows - 1)) * p.K * ESZ + KT::src_chunk_elems(row, lane) * 2u;
    }
#pragma unroll
    for (int i = 0; i < B_INST; ++i) {
        const int row = KTB::lane_row(w * B_INST + i, lane);
        const int j = GLU ? n0 + (row >> 6) * 32 + (row & 31) : n0 + row;   // gated: tile rows [64 wn + 32 half, +32) = packed columns [32 wn, +32)
        const int key = idxg[j < cnt ? j : n0];  // rows past the count re-read a live row and are never stored
        boff[i] = (uint32_t)key * p.K * BSZ + KTB::src_chunk_elems(row, lane) * 2u;
    }
    auto issue = [&](int kb, int buf) {
        unsigned char *st = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < A_INST; ++i) blds16(ra, aoff[i], kb * BK * 2, st + (w * A_INST + i) * 1024);
#pragma unroll
        for (int i = 0; i < B_INST; ++i) {
            if constexpr (GLU && W8) {   // pair (w * B_INST + i) >> 1 is wholly gate or wholly up (see above); W8's piece placement
                const bool up = (((w * B_INST + i) * KTB::RPI) >> 5) & 1;
                blds16(up ? rb_up : rb, boff[i], kb * BK, st + A_TILE + ((w * B_INST + i) >> 1) * B_PAIR + ((w * B_INST + i) & 1) * (1024 + 8));
            } else if constexpr (GLU) {
                const bool up = (((w * B_INST + i) * KT::RPI) >> 5) & 1;   // wave-uniform: the instruction's rows lie in one half
                blds16(up ? rb_up : rb, boff[i], kb * BK * 2, st + A_TILE + (w * B_INST + i) * 1024);
            } else if constexpr (W8) {   // BK bytes of a row per k step; the odd pieces land 8 bytes up
                blds16(rb, boff[i], kb * BK, st + A_TILE + ((w * B_INST + i) >> 1) * B_PAIR + ((w * B_INST + i) & 1) * (1024 + 8));
            } else {
                blds16(rb, boff[i], kb * BK * 2, st + A_TILE + (w * B_INST + i) * 1024);
            }
        }
    };
    // Epilogue operands staged through LDS when the tile's slice of the activation cache fits one ring stage: the
    // TN x TM block cache[idx[n0..], g*BM+m_off ..] (TN rows of TM*2 contiguous bytes) is fetched by LDS-DMA during
    // the LAST k step into the stage no tile needs any more, and the bf16 results leave through the other stage as
    // 16-byte row-major stores.  (Direct form: 8-byte gathered loads and 2-byte stores, 64 of each per lane --
    // measured 34 us of a 148 us launch.)
    // FLAT (tiles whose outputs exceed one stage): the ring starts at the stage that makes the LAST k step compute out of stage 0, the
    // cache block lands behind it in [STAGE, STAGE + TM*TN*2) and the outputs leave through stage 0 plus the bytes behind the cache block.
    constexpr int EPI = TM * PW * 2;   // (gated form: half the columns -- cache block PW columns x TM rows, output image TM x PW)
    // (W8: a stage is no whole number of output rows -- the rows behind the cache block start FLAT_SKIP behind their place in a contiguous image)
    constexpr int FLAT_ROWS = STAGE / (TN * 2), FLAT_SKIP = EPI + STAGE - FLAT_ROWS * TN * 2;
    constexpr bool FLAT = (NW == 8 || W8) && EPI > STAGE && EPI <= (NST - 1) * STAGE && EPI + FLAT_SKIP <= NST * STAGE &&
                          (W8 ? FLAT_ROWS % 4 == 0 : STAGE % (TN * 2) == 0);
    constexpr bool STAGED = EPI <= STAGE || FLAT;
    static_assert(!FP8 || STAGED, "the fp8 form is only built for tile shapes with the staged epilogue");
    static_assert(!GLU || (STAGED && !FLAT), "the gated form is only built for tile shapes with the staged epilogue");
    constexpr int LPR = TM * 2 / 16;                                  // 16-byte chunks per cache row
    constexpr int C_INST = STAGED ? EPI / (1024 * NW) : 1;            // DMA instructions per wave
    // The cache is [F, ldc]: a 16-byte piece that starts below M lies inside its column (ldc >= ceil8(M)), so the masks are
    // piece-granular; pieces that start at or past M re-read the column's first piece of this tile and are not written back.
    // (group-major, gs != BM: the G * gs = G * F * BM elements of the sequence's block)
    const __amdgpu_buffer_rsrc_t rc = make_rsrc(p.cache, (uint32_t)(p.gs == BM ? p.F * p.ldc : (p.M + BM - 1) / BM * p.gs) * 2u);
    uint32_t coff[C_INST];
    auto piece_row = [&](int jj) { return ((lane % LPR) ^ (jj & (LPR - 1))) << 3; };   // first tile row of the lane's piece of column jj
    if constexpr (STAGED) {
#pragma unroll
        for (int i = 0; i < C_INST; ++i) {
            const int jj = (w * C_INST + i) * (64 / LPR) + lane / LPR;  // tile-local packed column
            const int j = n0 + jj;
            const int col = idxg[j < cnt ? j : n0];
            const int ms = piece_row(jj);
            coff[i] = ((uint32_t)col * p.ldc + g * p.gs + m_off + (ms < rows ? ms : 0)) * 2u;
        }
    }
    auto issue_cache = [&](int buf) {
        if constexpr (STAGED) {
#pragma unroll
            for (int i = 0; i < C_INST; ++i) blds16(rc, coff[i], 0, smem + (FLAT ? STAGE : buf * STAGE) + (w * C_INST + i) * 1024);
        }
    };

    // bf16: the bias seeds the fp32 accumulators, as in the reference (csp_mlp_mm1.cu:347-350) -- its two dependent loads (index,
    // then bias) fly during the prologue instead of in front of the epilogue.  fp8 scales the sum first, so it starts from zero.
    constexpr bool SEED_BIAS = !FP8 && !W8;
    float bias_v[NT4], sa = 1.f, sb = 1.f;   // loaded here for both forms: in front of the epilogue the round trips would be exposed
    float sb_up = 1.f;                       // (gated fp8 form: sb is the gate weight's scale, sb_up the up weight's)
    float sb_col[RS || W8 ? NT4 : 1];        // (RS, W8: the weight scale of the lane's column of every 32-wide tile)
    if constexpr (FP8 && GLU) sa = p.scale_x[0], sb = p.scale_gate[0], sb_up = p.scale_up[0];
    else if constexpr (FP8 && !RS) sa = p.scale_a[0], sb = p.scale_b[0];
    f32x16 acc[MT][NT4];
#pragma unroll
    for (int n4 = 0; n4 < NT4; ++n4) {
        const int j = GLU ? n0 + wn * 32 + (lane & 31) : n0 + wn * (TN / WNC) + n4 * 32 + (lane & 31);
        if constexpr (GLU) {   // n4 = 0: the gate's bias, 1: the up projection's; a null vector is zero
            const uint16_t *bp = n4 ? p.bias_up : p.bias;
            bias_v[n4] = bp ? bf16_bits_to_f32(bp[idxg[j < cnt ? j : n0]]) : 0.f;
            if constexpr (W8) {   // the branch's reciprocal scale: one per weight row, gathered like the bias, or one number
                const float *sp = n4 ? p.scale_up : p.scale_gate;
                sb_col[n4] = sp[(n4 ? p.scale_up_n : p.scale_gate_n) > 1 ? idxg[j < cnt ? j : n0] : 0];
            }
        } else if constexpr (NULLB) {
            bias_v[n4] = p.bias ? bf16_bits_to_f32(p.bias[idxg[j < cnt ? j : n0]]) : 0.f;
            if constexpr (RS) sb_col[n4] = p.scale_b[idxg[j < cnt ? j : n0]];
            if constexpr (W8) sb_col[n4] = p.scale_b[p.scale_n > 1 ? idxg[j < cnt ? j : n0] : 0];   // one per fc1 row, or one number
        } else {
            bias_v[n4] = bf16_bits_to_f32(p.bias[idxg[j < cnt ? j : n0]]);
        }
        const float seed = SEED_BIAS ? bias_v[n4] : 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][n4][r] = seed;
    }

    const int nkb = (int)((uint32_t)p.K * ESZ / (BK * 2));
    int buf = FLAT ? (NST - (nkb - 1) % NST) % NST : 0;   // FLAT: k step nkb-1 computes out of stage 0
    // W8: every register load of the tile -- gather indices, bias, scale -- has landed before the first LDS-DMA is issued, so none of them is
    // consumed under a counted vmcnt with LDS-DMAs behind it (an LDS-DMA may retire ahead of an older register load).  The counted
    // waits the compiler still puts in front of their uses then wait for nothing; the loop and the epilogue issue no register load of their own.
    if constexpr (W8) wait_vmcnt<0>();
#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
        if (s < nkb) issue(s, (buf + s) % NST);
    int nbuf = (buf + NST - 1) % NST;
    MPROF_DECL;
    MPROF_ABS(1);
    MPROF_START();
    for (int kb = 0; kb < nkb; ++kb) {
        // tile kb must have landed; the NST-2 younger tiles may stay in flight across the barrier
        if (kb + NST - 1 <= nkb) wait_vmcnt<(NST - 2) * (A_INST + B_INST)>();
        else wait_vmcnt<0>();
        MPROF_MARK(0);
        __builtin_amdgcn_s_barrier();
        MPROF_MARK(1);
        if (kb + NST - 1 < nkb && p.probe != 1) issue(kb + NST - 1, nbuf);
        if (kb == nkb - 1) issue_cache(nbuf);  // the stage tile kb-1 occupied is free for good
        MPROF_MARK(2);
        if (p.probe == 2) {
            buf = buf + 1 == NST ? 0 : buf + 1;
            nbuf = nbuf + 1 == NST ? 0 : nbuf + 1;
            continue;
        }
        const unsigned char *At = smem + buf * STAGE;
        const unsigned char *Bt = At + A_TILE;
        // operand fragments are double-buffered in registers: the ds_reads of k-slice kk+1 are in flight while the
        // MFMAs of slice kk issue (left to itself hipcc emits read -> lgkmcnt(0) -> 4 MFMA -> read ...)
        // one MFMA k slice: bf16 = 16 elements (v_mfma_f32_32x32x16_bf16: 32 bytes of a row, 16 per lane half); fp8 = 64 elements
        // (v_mfma_f32_32x32x64_f8f6f4, the K = 64 form that runs e4m3 at twice the bf16 rate -- the K = 16 fp8 MFMA runs at the
        // bf16 rate: 64 bytes of a row, 32 per lane half = two 16-byte chunks, each swizzled on its own).  A and B fetch the same
        // chunk positions of their rows, so the pairing of k elements inside the instruction is the same on both sides whatever
        // order the hardware walks them in.
        typedef __attribute__((ext_vector_type(8))) int i32x8;
        constexpr int KK = FP8 ? BK * 2 / 64 : BK / 16;
        using Frag = typename std::conditional<FP8, i32x8, bf16x8>::type;
        Frag af[2][MT], bfr[2][NT4];
        u32x2 bw8[2][W8 ? NT4 : 1];   // (W8: the fragments' e4m3 bytes, widened in front of their MFMAs)
        auto frag = [&](const unsigned char *tile, int row, int kk) -> Frag {
            if constexpr (FP8) {
                const int c0 = kk * 4 + (lane >> 5) * 2;
                const u32x4 lo = *(const u32x4 *)(tile + row * (BK * 2) + ((c0 ^ KT::swz(row)) << 4));
                const u32x4 hi = *(const u32x4 *)(tile + row * (BK * 2) + (((c0 + 1) ^ KT::swz(row)) << 4));
                return (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            } else {
                return KT::frag(tile, row, kk, lane);
            }
        };
        auto load_frags = [&](int kk, int set) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) af[set][mt] = frag(At, wm * (TM / 2) + mt * 32 + (lane & 31), kk);
#pragma unroll
            for (int n4 = 0; n4 < NT4; ++n4) {
                const int row = wn * (TN / WNC) + n4 * 32 + (lane & 31);
                if constexpr (W8)
                    bw8[set][n4] = *(const u32x2 *)(Bt + (row >> 5) * B_PAIR + ((row >> 4) & 1) * (1024 + 8) + (row & 15) * KTB::ROWB +
                                                    ((kk ^ KTB::swz(row)) << 4) + (lane >> 5) * 8);
                else
                    bfr[set][n4] = frag(Bt, row, kk);
            }
        };
        load_frags(0, 0);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            if (kk + 1 < KK) load_frags(kk + 1, (kk + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);  // keep the next slice's reads ahead of this slice's MFMAs
            if constexpr (W8) {
#pragma unroll
                for (int n4 = 0; n4 < NT4; ++n4) {
                    const u32x2 r = bw8[kk & 1][n4];
                    const bf16x2 f0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[0], 1.0f, false), f1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[0], 1.0f, true);
                    const bf16x2 f2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[1], 1.0f, false), f3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[1], 1.0f, true);
                    bfr[kk & 1][n4] = (bf16x8){f0[0], f0[1], f1[0], f1[1], f2[0], f2[1], f3[0], f3[1]};
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int n4 = 0; n4 < NT4; ++n4) {
                    if constexpr (FP8)   // formats 0 / 0 = e4m3 x e4m3; literal zero scale operands select the unscaled encoding
                        acc[mt][n4] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[kk & 1][mt], bfr[kk & 1][n4], acc[mt][n4], 0, 0, 0, 0, 0, 0);
                    else
                        acc[mt][n4] = mfma32(af[kk & 1][mt], bfr[kk & 1][n4], acc[mt][n4]);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        MPROF_MARK(3);
        buf = buf + 1 == NST ? 0 : buf + 1;
        nbuf = nbuf + 1 == NST ? 0 : nbuf + 1;
    }
    MPROF_MARK(4);

    if (p.probe == 4) {  // timing probe: no epilogue
        float t = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int n4 = 0; n4 < NT4; ++n4)
#pragma unroll
                for (int r = 0; r < 16; ++r) t += acc[mt][n4][r];
        if (t == 123.456f) p.c[0] = 1;
        return;
    }
    // ---- epilogue: lane owns packed column j = lane&31 of each 32x32 tile and rows (r&3) + 8*(r>>2) + 4*(lane>>5)
    //      C[m,j] = bf16(gelu(acc + bias[idx]) - cache[idx, m])     (csp_mlp_mm1.cu:354-390)
    if constexpr (STAGED) {
        // after the loop: buf = stage after the last computed one = the cache stage (NST = 2) or a free one
        const int last = buf == 0 ? NST - 1 : buf - 1;                  // stage of tile nkb-1
        const int cst = last + NST - 1 >= NST ? last - 1 : last + NST - 1;  // nbuf at kb = nkb-1
        unsigned char *Ct = smem + (FLAT ? 1 : cst) * STAGE, *Ot = smem + (FLAT ? 0 : last) * STAGE;
        // output row r of the stage image (FLAT: the rows that do not fit stage 0 continue behind the cache block)
        auto ot_row = [&](int r) { return Ot + r * (PW * 2) + ((FLAT && r >= FLAT_ROWS) ? FLAT_SKIP : 0); };
        constexpr int LPO = PW * 2 / 16;  // 16-byte chunks per output row
        // RS: the reciprocal scales of the lane's rows, runs of four (ml .. ml + 3 per (mt, q4)), requested here so that they land under the
        // wait for the cache block.  M % 4 == 0 and a 16-byte aligned vector (wave-uniform): a run is live or dead as a whole and arrives as
        // one 16-byte read, a dead run re-reads the tile's last live one; otherwise four reads, each row clamped to the last live row.
        f32x4 sa_row[RS ? MT : 1][RS ? 4 : 1];
        if constexpr (RS) {
            const float *sap = p.scale_a + (g * BM + m_off);
            const bool vec = (p.M & 3) == 0 && ((uintptr_t)p.scale_a & 15) == 0;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const int ml = wm * (TM / 2) + mt * 32 + q4 * 8 + (lane >> 5) * 4;
                    if (vec) {
                        sa_row[mt][q4] = *(const f32x4 *)(sap + min(ml, rows - 4));
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) sa_row[mt][q4][e] = sap[min(ml + e, rows - 1)];
                    }
                }
        }
        wait_vmcnt<0>();
        __syncthreads();  // cache block landed; every wave is done reading the last tile
        // The output stage is plain row-major: a ds_write_b16 puts 32 consecutive columns of one row (64 contiguous bytes) per half
        // wave, and the 16-byte read-back below walks whole rows, so neither side needs a swizzle (the cache block does: its 32 lanes
        // of a read hit 32 rows of the [column][m] image at one m).  Two values per instruction wherever the ISA has a packed form.
        // The arithmetic is specialised on update_cache (three straight-line copies: with a branch per element group hipcc serialises the groups,
        // one exposed LDS round trip each) and reads the cache values of a whole 32-column tile ahead of that tile's arithmetic.
        auto arith = [&](auto upd_) {
            constexpr int UPD = decltype(upd_)::value;
            u32x2 cv[2][MT][4];
            auto cptr = [&](int n4, int mt, int q4) {
                const int jl = wn * (PW / WNC) + n4 * 32 + (lane & 31), ml = wm * (TM / 2) + mt * 32 + q4 * 8 + (lane >> 5) * 4;
                return Ct + jl * (TM * 2) + (((ml >> 3) ^ (jl & (LPR - 1))) << 4) + (ml & 7) * 2;
            };
            auto load = [&](int n4) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) cv[n4 & 1][mt][q4] = *(const u32x2 *)cptr(n4, mt, q4);
            };
            load(0);
#pragma unroll
            for (int n4 = 0; n4 < NP4; ++n4) {
                if (n4 + 1 < NP4) load(n4 + 1);
                const int jl = wn * (PW / WNC) + n4 * 32 + (lane & 31);
                const float bia = bias_v[n4];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        const int ml = wm * (TM / 2) + mt * 32 + q4 * 8 + (lane >> 5) * 4;
                        const u32x2 c = cv[n4 & 1][mt][q4];
                        const f32x2 c01 = unpack_bf16x2(c[0]), c23 = unpack_bf16x2(c[1]);
                        f32x2 a01 = {acc[mt][n4][q4 * 4 + 0], acc[mt][n4][q4 * 4 + 1]}, a23 = {acc[mt][n4][q4 * 4 + 2], acc[mt][n4][q4 * 4 + 3]};
                        uint32_t d01, d23, n01 = 0, n23 = 0;   // packed deltas as stored (bf16 pairs); the cache block's new values
                        if constexpr (FP8 && GLU) {
                            // each branch as the fp8 form makes its pre-activation, (acc * scale_a) * scale_b + bias, then the gated form's
                            // one rounding: fma(act(gate), up, -cache); a01 / a23 are the gate's sums, bias_v[1] the up projection's bias
                            const f32x2 u01 = {acc[mt][1][q4 * 4 + 0], acc[mt][1][q4 * 4 + 1]}, u23 = {acc[mt][1][q4 * 4 + 2], acc[mt][1][q4 * 4 + 3]};
                            const f32x2 sav = {sa, sa}, sgv = {sb, sb}, suv = {sb_up, sb_up}, bgv = {bia, bia}, buv = {bias_v[1], bias_v[1]};
                            d01 = pack_bf16x2_v(__builtin_elementwise_fma(glu_act2<ACT>((a01 * sav) * sgv + bgv), (u01 * sav) * suv + buv, -c01));
                            d23 = pack_bf16x2_v(__builtin_elementwise_fma(glu_act2<ACT>((a23 * sav) * sgv + bgv), (u23 * sav) * suv + buv, -c23));
                        } else if constexpr (FP8) {
                            // (acc * scale_a) * scale_b + bias in the reference's order -> gelu -> bf16, then a bf16 subtract (csp_mlp_mm1.py:121-133)
                            f32x2 sav = {sa, sa}, sav23 = {sa, sa}, sbv = {sb, sb};
                            if constexpr (RS) {   // the rows' own scales, the gathered column's
                                sav = (f32x2){sa_row[mt][q4][0], sa_row[mt][q4][1]}, sav23 = (f32x2){sa_row[mt][q4][2], sa_row[mt][q4][3]};
                                sbv = (f32x2){sb_col[n4], sb_col[n4]};
                            }
                            const f32x2 bv = {bia, bia};
                            const uint32_t t01 = pack_bf16x2_v(glu_act2<ACT>((a01 * sav) * sbv + bv));
                            const uint32_t t23 = pack_bf16x2_v(glu_act2<ACT>((a23 * sav23) * sbv + bv));
                            d01 = pack_bf16x2_v(unpack_bf16x2(t01) - c01), d23 = pack_bf16x2_v(unpack_bf16x2(t23) - c23);
                            if constexpr (UPD == 2) n01 = t01, n23 = t23;   // 2: cache = new activation, what the reference's Triton kernel does (csp_mlp_mm1.py:140)
                        } else if constexpr (GLU && W8) {
                            // each branch: sum * scale, then + bias, two roundings each (scale_then_bias2); then the gated form's one rounding
                            const f32x2 u01 = {acc[mt][1][q4 * 4 + 0], acc[mt][1][q4 * 4 + 1]}, u23 = {acc[mt][1][q4 * 4 + 2], acc[mt][1][q4 * 4 + 3]};
                            const f32x2 sgv = {sb_col[0], sb_col[0]}, suv = {sb_col[1], sb_col[1]}, bgv = {bia, bia}, buv = {bias_v[1], bias_v[1]};
                            d01 = pack_bf16x2_v(__builtin_elementwise_fma(glu_act2<ACT>(scale_then_bias2(a01, sgv, bgv)), scale_then_bias2(u01, suv, buv), -c01));
                            d23 = pack_bf16x2_v(__builtin_elementwise_fma(glu_act2<ACT>(scale_then_bias2(a23, sgv, bgv)), scale_then_bias2(u23, suv, buv), -c23));
                        } else if constexpr (GLU) {
                            // act(gate) * up - cache in fp32, one rounding (both biases are already in the sums); a01 / a23 are the gate's
                            const f32x2 u01 = {acc[mt][1][q4 * 4 + 0], acc[mt][1][q4 * 4 + 1]}, u23 = {acc[mt][1][q4 * 4 + 2], acc[mt][1][q4 * 4 + 3]};
                            d01 = pack_bf16x2_v(__builtin_elementwise_fma(glu_act2<ACT>(a01), u01, -c01));
                            d23 = pack_bf16x2_v(__builtin_elementwise_fma(glu_act2<ACT>(a23), u23, -c23));
                        } else if constexpr (W8) {
                            // sum * scale, then + bias: two fp32 roundings (scale_then_bias2), then the bf16 form's one rounding
                            const f32x2 sbv = {sb_col[n4], sb_col[n4]}, bv = {bia, bia};
                            d01 = pack_bf16x2_v(glu_act2<ACT>(scale_then_bias2(a01, sbv, bv)) - c01);
                            d23 = pack_bf16x2_v(glu_act2<ACT>(scale_then_bias2(a23, sbv, bv)) - c23);
                        } else {
                            // the bias is already in the sum (SEED_BIAS)
                            d01 = pack_bf16x2_v(glu_act2<ACT>(a01) - c01), d23 = pack_bf16x2_v(glu_act2<ACT>(a23) - c23);
                        }
                        uint16_t *op = (uint16_t *)(ot_row(ml) + jl * 2);   // (rows ml .. ml+3: on one side of the split, a multiple of 4)
                        op[0] = (uint16_t)d01, op[PW] = (uint16_t)(d01 >> 16), op[2 * PW] = (uint16_t)d23, op[3 * PW] = (uint16_t)(d23 >> 16);
                        if constexpr (UPD != 0) {
                            // 1: cache += delta in bf16, exactly what csp_scatter_add does (scatter_add.cu:43-98)
                            if constexpr (!(FP8 && UPD == 2))
                                n01 = pack_bf16x2_v(c01 + unpack_bf16x2(d01)), n23 = pack_bf16x2_v(c23 + unpack_bf16x2(d23));
                            *(u32x2 *)cptr(n4, mt, q4) = (u32x2){n01, n23};
                        }
                    }
                }
            }
        };
        if (p.update_cache == 0) arith(ic<0>{});
        else if constexpr (GLU || W8) arith(ic<1>{});   // (the gated and the weight-only entries admit 0 and 1 only: no third copy of the epilogue)
        else if (p.update_cache == 1) arith(ic<1>{});
        else arith(ic<2>{});
        __syncthreads();
        constexpr int O_INST = EPI / (1024 * NW);  // 1 KiB row-major pieces per wave
#pragma unroll
        for (int i = 0; i < O_INST; ++i) {
            const int r = (w * O_INST + i) * (64 / LPO) + lane / LPO, ch = lane % LPO;
            const u32x4 v = *(const u32x4 *)(ot_row(r) + (ch << 4));
            const int j = n0 + ch * 8;
            uint16_t *cp = p.c + (int64_t)(g * BM + m_off + r) * p.F + j;
            if (r >= rows) continue;   // ragged last group: no row at or past M is stored
            if (j + 8 <= cnt && (p.F & 7) == 0) {
                *(u32x4 *)cp = v;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (j + e < cnt) cp[e] = (uint16_t)(v[e >> 1] >> ((e & 1) * 16));
            }
        }
        if (p.update_cache) {  // the updated cache block goes back the way it came: 1 KiB pieces, TM*2-byte row segments
#pragma unroll
            for (int i = 0; i < C_INST; ++i) {
                const int jj = (w * C_INST + i) * (64 / LPR) + lane / LPR;
                const int ms = piece_row(jj);
                if (n0 + jj < cnt && ms < rows) {
                    const u32x4 v = *(const u32x4 *)(Ct + (w * C_INST + i) * 1024 + lane * 16);
                    if (ms + 8 <= rows) {
                        *(u32x4 *)((unsigned char *)p.cache + coff[i]) = v;
                    } else {   // the piece that straddles M: the elements at or past M (the padding of a pitched cache) keep what they hold
                        uint16_t *cp = (uint16_t *)((unsigned char *)p.cache + coff[i]);
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (ms + e < rows) cp[e] = (uint16_t)(v[e >> 1] >> ((e & 1) * 16));
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int n4 = 0; n4 < NT4; ++n4) {
            const int j = n0 + wn * (TN / WNC) + n4 * 32 + (lane & 31);
            const bool live = j < cnt;
            const int col = live ? idxg[j] : 0;
            const uint16_t *crow = p.cache + (int64_t)col * p.ldc + (int64_t)g * (p.gs - BM);   // (+ m below: g * BM of it is in m)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const int m = g * BM + m_off + wm * (TM / 2) + mt * 32 + q4 * 8 + (lane >> 5) * 4;
                    const u32x2 cv = *(const u32x2 *)(crow + m);
                    const float c0 = __uint_as_float(cv[0] << 16), c1 = __uint_as_float(cv[0] & 0xffff0000u);
                    const float c2 = __uint_as_float(cv[1] << 16), c3 = __uint_as_float(cv[1] & 0xffff0000u);
                    const float x0 = glu_act<ACT>(acc[mt][n4][q4 * 4 + 0]) - c0;   // (bias already in the sum)
                    const float x1 = glu_act<ACT>(acc[mt][n4][q4 * 4 + 1]) - c1;
                    const float x2 = glu_act<ACT>(acc[mt][n4][q4 * 4 + 2]) - c2;
                    const float x3 = glu_act<ACT>(acc[mt][n4][q4 * 4 + 3]) - c3;
                    if (live) {
                        uint16_t *cp = p.c + (int64_t)m * p.F + j;
                        cp[0] = f32_to_bf16_bits(x0);
                        cp[(int64_t)p.F] = f32_to_bf16_bits(x1);
                        cp[2 * (int64_t)p.F] = f32_to_bf16_bits(x2);
                        cp[3 * (int64_t)p.F] = f32_to_bf16_bits(x3);
                    }
                }
            }
        }
    }
#ifdef MLP_PROF
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    MPROF_ABS(2);
    MPROF_MARK(5);   // epilogue (mark 4 = loop exit edge)
    MPROF_END(w, nkb);
}

// Batched launch (B > 1 sequences in one grid): the operands of sequence b are its slices of dense [B, M, .] tensors, the cache
// [B, F, ldc] with a batch stride of its own; indices [B, G, F] and counts [B, G] are the per-sequence lists back to back, i.e. one list
// of B * G groups.  The tile map runs over those B * G groups (group g = sequence g / G, local group g % G), and a tile then sees the
// Mm1Params of ITS sequence: base pointers advanced in 64-bit arithmetic, so the descriptors keep per-sequence sizes and every 32-bit
// offset inside a sequence stays what it is in a single-sequence launch.  Every output element is still produced by one workgroup in
// the same K order: the bits of B separate launches.
struct Mm1Batch : Mm1Params {
    int B;
    int64_t cache_bs;   // elements between the caches of consecutive sequences (>= F * ldc)
};
struct Mm1GluF8Batch : Mm1GluF8Params {
    int B;
    int64_t cache_bs;   // as Mm1Batch
};
// (the gated fp8 form?, batched?) -> the parameter block a kernel takes
template <bool F8GLU, bool BATCHED> struct Mm1Block { using type = typename std::conditional<BATCHED, Mm1Batch, Mm1Params>::type; };
template <bool BATCHED> struct Mm1Block<true, BATCHED> { using type = typename std::conditional<BATCHED, Mm1GluF8Batch, Mm1GluF8Params>::type; };

template <int BN, int BK, int NST, int WPS, bool FP8 = false, int NW = 4, bool BATCHED = false>
__global__ __launch_bounds__(NW * 64, WPS) void mm1_kernel(const typename std::conditional<BATCHED, Mm1Batch, Mm1Params>::type p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MPROF_ABS(0);
    constexpr int NSUB = NW == 4 ? 2 * (BN / 64) : 1;  // 64 x 64 sub-tiles per tile (the 8-wave form has no tail split)
    // PERSISTENT workgroups: the grid is the resident slots (WPS per CU); a workgroup walks its XCD's tile list with the stride of the
    // XCD's slots -- the same tile-to-slot order a one-tile-per-workgroup grid is dispatched in, without the relaunch between tiles
    // (kernel arguments, the live-tile map, wave start-up: 5.4 k of a 41 k-cycle tile at the Wan2.1 fp8 shape, tools/mlp_prof.py) and
    // with the previous tile's stores draining under the next tile's index loads.  (Requesting the NEXT tile's gather indices during
    // the current tile -- one exposed round trip less -- measured no gain at the fp8 shape, 209 vs 209-224 us, for 40 more registers.)
    const int Gs = (p.M + BM - 1) / BM;   // groups of one sequence
    int G = Gs;
    if constexpr (BATCHED) G = p.B * Gs;  // the map runs over all B * Gs
    const TilePlan pl = plan_tiles<BN>(p.counts, G, p.NT, p.NR, p.slots_per_xcd, NSUB);
    const int nslots = pl.slots(), stride = (int)(gridDim.x >> 3);
    for (int slot = blockIdx.x >> 3; slot < nslots; slot += stride) {
        const TileMap tm = tile_at(pl, slot);
        if (!tm.live) continue;
        const int cnt = p.counts[tm.g];
        int g = tm.g;
        typename std::conditional<BATCHED, Mm1Params, const Mm1Params &>::type q = p;   // the tile sees its sequence's operands
        if constexpr (BATCHED) {
            const int b = tm.g / Gs;
            g = tm.g - b * Gs;                        // group inside sequence b
            q.a = (const uint16_t *)((const unsigned char *)p.a + (int64_t)b * p.M * p.K * (FP8 ? 1 : 2));
            q.c = p.c + (int64_t)b * p.M * p.F;
            q.cache = p.cache + (int64_t)b * p.cache_bs;
            q.indices = p.indices + (int64_t)b * Gs * p.F;
        }
        if (tm.sub < 0) {
            const int n0 = tm.nt * BN;
            if (n0 >= cnt) continue;  // tiles past counts[g] are skipped (csp_mlp_mm1.cu:233-243)
            mm1_tile<BM, BN, BK, NST, FP8, NW>(q, smem, g, 0, n0, cnt);
        } else if constexpr (NW == 4) {
            constexpr int SUB_NST = (NST * (BM + BN)) / 128;  // same LDS bytes, stages of 64 + 64 rows
            const int n0 = tm.nt * BN + (tm.sub >> 1) * 64;
            if (n0 >= cnt || p.probe == 3) continue;  // probe 3: time the launch without its tail
            if (g * BM + (tm.sub & 1) * 64 >= p.M) continue;   // ragged last group: no row of this sub-tile exists
            mm1_tile<64, 64, BK, (SUB_NST > 4 ? 4 : SUB_NST), FP8>(q, smem, g, (tm.sub & 1) * 64, n0, cnt);
        }
        __syncthreads();   // the next tile's DMA lands where this tile's epilogue was reading
    }
}

// Every GEMM1 form but mm1_kernel's (4 waves, the shipped tile shape's walk): the persistent walk over the live-tile map, the ragged last
// group and the batch pointer advance written once, mm1_tile's form chosen by the flags:
//   FP8      e4m3 operands (a sequence of a batch then starts M * K bytes behind the one before, not 2 * M * K);
//   GLU      the gated form: a whole tile covers BN / 2 packed columns, no tail split (slots_per_xcd is not read: the launch is correct either
//            way), tiles past counts[g] are skipped BEFORE the batch advance; with FP8 the parameter block is Mm1GluF8Params (Mm1Block);
//   ACT      CHIPMUNK_ACT_*; the ungated forms also read a null bias as zero (mm1_tile's NULLB);
//   RS       (ungated fp8) scale_a / scale_b are vectors; scale_a is [B, M] for a batch and advances with the sequence;
//   BATCHED  the parameter block carries B and cache_bs, and a tile sees its sequence's operands; otherwise the kernel's own block.
// mm1_kernel stays a kernel of its own: the benchmark times it, it carries the MLP_PROF marks, probe == 3 and the 8-wave / probe-build
// shapes, and a walk shared with other instantiations through a device function moved its scalar register allocation.  The order of the
// statements below is the order each form's code was first compiled from (tools/mlp_isa_diff.py compares the instruction streams).
template <int BN, int BK, int NST, int WPS, bool FP8, bool GLU, int ACT, bool RS, bool BATCHED>
__global__ __launch_bounds__(256, WPS) void mm1_form_kernel(const typename Mm1Block<FP8 && GLU, BATCHED>::type p) {
    using P = typename Mm1Block<FP8 && GLU, false>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int PBN = GLU ? BN / 2 : BN;            // packed columns of a whole tile: the gated B tile's BN rows are {gate, up} pairs
    constexpr int NSUB = GLU ? 1 : 2 * (BN / 64);     // 64 x 64 sub-tiles per tile
    constexpr int SUB_NST = (NST * (BM + BN)) / 128 > 4 ? 4 : (NST * (BM + BN)) / 128;  // same LDS bytes, stages of 64 + 64 rows
    const int Gs = (p.M + BM - 1) / BM;   // groups of one sequence
    int G = Gs;
    if constexpr (BATCHED) G = p.B * Gs;  // the map runs over all B * Gs
    const TilePlan pl = plan_tiles<PBN>(p.counts, G, p.NT, p.NR, GLU ? 0 : p.slots_per_xcd, NSUB);
    const int nslots = pl.slots(), stride = (int)(gridDim.x >> 3);
    for (int slot = blockIdx.x >> 3; slot < nslots; slot += stride) {
        const TileMap tm = tile_at(pl, slot);
        if (!tm.live) continue;
        const int cnt = p.counts[tm.g];
        if constexpr (GLU) {
            if (tm.nt * PBN >= cnt) continue;  // tiles past counts[g] are skipped
        }
        int g = tm.g;
        // the tile sees its sequence's operands (a gated single sequence: the kernel's own block, no copy -- the copy costs it SGPR spills)
        typename std::conditional<BATCHED || !GLU, P, const P &>::type q = p;
        if constexpr (BATCHED) {
            const int b = tm.g / Gs;
            g = tm.g - b * Gs;                        // group inside sequence b
            if constexpr (GLU && !FP8) q.a = p.a + (int64_t)b * p.M * p.K;   // (in elements: in bytes this form compiles to other code)
            else q.a = (const uint16_t *)((const unsigned char *)p.a + (int64_t)b * p.M * p.K * (FP8 ? 1 : 2));
            q.c = p.c + (int64_t)b * p.M * p.F;
            q.cache = p.cache + (int64_t)b * p.cache_bs;
            q.indices = p.indices + (int64_t)b * Gs * p.F;
            if constexpr (RS) q.scale_a = p.scale_a + (int64_t)b * p.M;   // [B, M]: the sequence's row scales
        }
        if constexpr (GLU) {
            mm1_tile<BM, BN, BK, NST, FP8, 4, true, ACT, P>(q, smem, g, 0, tm.nt * PBN, cnt);
        } else if (tm.sub < 0) {
            const int n0 = tm.nt * BN;
            if (n0 >= cnt) continue;  // tiles past counts[g] are skipped
            mm1_tile<BM, BN, BK, NST, FP8, 4, false, ACT, P, true, RS>(q, smem, g, 0, n0, cnt);
        } else {
            const int n0 = tm.nt * BN + (tm.sub >> 1) * 64;
            if (n0 >= cnt) continue;
            if (g * BM + (tm.sub & 1) * 64 >= p.M) continue;   // ragged last group: no row of this sub-tile exists
            mm1_tile<64, 64, BK, SUB_NST, FP8, 4, false, ACT, P, true, RS>(q, smem, g, (tm.sub & 1) * 64, n0, cnt);
        }
        __syncthreads();   // the next tile's DMA lands where this tile's epilogue was reading
    }
}


#ifndef CHIPMUNK_MM1_PROBES
// Weight-only e4m3 fc1 (mm1_tile's W8 form): c = bf16(act((a . f(b[i, :])) * scale_b[i] + bias[i]) - cache[i, m]) with bf16 a and f the exact
// e4m3 -> bf16 widening.  mm1_form_kernel's walk for an ungated form -- live-tile map, tail split into 64 x 64 sub-tiles, ragged last group,
// batch pointer advance -- under a name of its own.  A stage is 16 KiB of A + 8 KiB of B (+ 64), smaller than the 32 KiB images of the staged
// epilogue, so the whole tile runs NST = 3 stages with mm1_tile's FLAT epilogue: the last k step computes out of stage 0, the cache block
// lands in the two stages behind it, and the outputs leave through stage 0 and the bytes behind the cache block.
struct Mm1W8Batch : Mm1W8Params {
    int B;
    int64_t cache_bs;   // as Mm1Batch
};
template <int BN, int BK, int NST, int WPS, int ACT, bool BATCHED>
__global__ __launch_bounds__(256, WPS) void mm1_w8_kernel(const typename std::conditional<BATCHED, Mm1W8Batch, Mm1W8Params>::type p) {
    using P = Mm1W8Params;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NSUB = 2 * (BN / 64);                                   // 64 x 64 sub-tiles per tile
    constexpr int LDS = NST * (BM * BK * 2 + BN * BK + BN / 32 * 16), SUB_STAGE = 64 * BK * 2 + 64 * BK + 32;
    constexpr int SUB_NST = LDS / SUB_STAGE > 4 ? 4 : LDS / SUB_STAGE;    // inside the same LDS bytes
    const int Gs = (p.M + BM - 1) / BM;   // groups of one sequence
    int G = Gs;
    if constexpr (BATCHED) G = p.B * Gs;  // the map runs over all B * Gs
    const TilePlan pl = plan_tiles<BN>(p.counts, G, p.NT, p.NR, p.slots_per_xcd, NSUB);
    const int nslots = pl.slots(), stride = (int)(gridDim.x >> 3);
    for (int slot = blockIdx.x >> 3; slot < nslots; slot += stride) {
        const TileMap tm = tile_at(pl, slot);
        if (!tm.live) continue;
        const int cnt = p.counts[tm.g];
        int g = tm.g;
        typename std::conditional<BATCHED, P, const P &>::type q = p;   // the tile sees its sequence's operands (one sequence: the kernel's own block)
        if constexpr (BATCHED) {
            const int seq = tm.g / Gs;
            g = tm.g - seq * Gs;                      // group inside sequence seq
            q.a = p.a + (int64_t)seq * p.M * p.K;
            q.c = p.c + (int64_t)seq * p.M * p.F;
            q.cache = p.cache + (int64_t)seq * p.cache_bs;
            q.indices = p.indices + (int64_t)seq * Gs * p.F;
        }
        if (tm.sub < 0) {
            const int n0 = tm.nt * BN;
            if (n0 >= cnt) continue;  // tiles past counts[g] are skipped
            mm1_tile<BM, BN, BK, NST, false, 4, false, ACT, P, true, false, true>(q, smem, g, 0, n0, cnt);
        } else {
            const int n0 = tm.nt * BN + (tm.sub >> 1) * 64;
            if (n0 >= cnt) continue;
            if (g * BM + (tm.sub & 1) * 64 >= p.M) continue;   // ragged last group: no row of this sub-tile exists
            mm1_tile<64, 64, BK, SUB_NST, false, 4, false, ACT, P, true, false, true>(q, smem, g, (tm.sub & 1) * 64, n0, cnt);
        }
        __syncthreads();   // the next tile's DMA lands where this tile's epilogue was reading
    }
}

// Gated weight-only e4m3 gate / up (mm1_tile's GLU && W8 form): c = bf16(fma(act(g), u, -cache[i, m])), g = (a . f(b[i, :])) * scale_gate[i] +
// bias[i], u the same over b_up / scale_up / bias_up.  mm1_form_kernel's walk for a gated form -- a whole tile is BN / 2 packed columns, no tail
// split, tiles past counts[g] skipped before the batch advance, the single sequence on the kernel's own block -- under a name of its own.
struct Mm1GluW8Batch : Mm1GluW8Params {
    int B;
    int64_t cache_bs;   // as Mm1Batch
};
template <int BN, int BK, int NST, int WPS, int ACT, bool BATCHED>
__global__ __launch_bounds__(256, WPS) void mm1_glu_w8_kernel(const typename std::conditional<BATCHED, Mm1GluW8Batch, Mm1GluW8Params>::type p) {
    using P = Mm1GluW8Params;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int PBN = BN / 2;           // packed columns of a whole tile: the B tile's BN rows are {gate, up} pairs
    const int Gs = (p.M + BM - 1) / BM;   // groups of one sequence
    int G = Gs;
    if constexpr (BATCHED) G = p.B * Gs;  // the map runs over all B * Gs
    const TilePlan pl = plan_tiles<PBN>(p.counts, G, p.NT, p.NR, 0, 1);   // (no tail split)
    const int nslots = pl.slots(), stride = (int)(gridDim.x >> 3);
    for (int slot = blockIdx.x >> 3; slot < nslots; slot += stride) {
        const TileMap tm = tile_at(pl, slot);
        if (!tm.live) continue;
        const int cnt = p.counts[tm.g];
        if (tm.nt * PBN >= cnt) continue;  // tiles past counts[g] are skipped
        int g = tm.g;
        typename std::conditional<BATCHED, P, const P &>::type q = p;   // the tile sees its sequence's operands (one sequence: the kernel's own block)
        if constexpr (BATCHED) {
            const int seq = tm.g / Gs;
            g = tm.g - seq * Gs;                      // group inside sequence seq
            q.a = p.a + (int64_t)seq * p.M * p.K;
            q.c = p.c + (int64_t)seq * p.M * p.F;
            q.cache = p.cache + (int64_t)seq * p.cache_bs;
            q.indices = p.indices + (int64_t)seq * Gs * p.F;
        }
        mm1_tile<BM, BN, BK, NST, false, 4, true, ACT, P, false, false, true>(q, smem, g, 0, tm.nt * PBN, cnt);
        __syncthreads();   // the next tile's DMA lands where this tile's epilogue was reading
    }
}
#endif   // CHIPMUNK_MM1_PROBES

// The tile shapes and producer / consumer forms measured against the shipped kernels (docs/EXPERIMENTS_r04.md / _r05.md) are
// not part of the product library: tools/probes/mm1_forms/build.sh compiles this file with -DCHIPMUNK_MM1_PROBES into
// tools/bin/forms/libchipmunk_hip.so, where options mm1_variant / mm2_variant select them (same parity tests, tests/test_gpu_mlp_forms.py).
#ifdef CHIPMUNK_MM1_PROBES
#include "mlp_pc.h"
#include "mlp_pp.h"
#endif

// ------------------------------------------------------------------------------------------------ mm2
struct Mm2Params {
    const uint16_t *a, *b;  // a = packed [M,F], b = fc2^T [F,N2]
    uint16_t *c;            // [M,N2], accumulated in place
    const int32_t *indices, *counts;
    int M, F, N2, NT, NR, probe;
    int cus_per_xcd;   // > 0: length-aware placement of a one-round launch (see mm2_kernel), 0: dispatch order = tile order
};

// Batched launch: as Mm1Batch -- a [B, M, F], c [B, M, N2], indices [B, G, F], counts [B, G]; the map runs over B * G groups
struct Mm2Batch : Mm2Params {
    int B;
};

template <int BN, int BK, int NST, int WPS, int NW = 4, bool BATCHED = false>
__global__ __launch_bounds__(NW == 8 ? 512 : 256, WPS) void mm2_kernel(const typename std::conditional<BATCHED, Mm2Batch, Mm2Params>::type p) {
    static_assert(NW == 4 || NW == 8, "4 waves (2 x 2) or 8 waves (2 x 4)");
    constexpr int WNG = NW / 2;                 // waves along n; wave tile = 64 rows x BN/WNG columns
    using KT = KTile<BK>;
    constexpr int A_TILE = BM * BK * 2, B_TILE = BK * BN * 2, STAGE = A_TILE + B_TILE;
    constexpr int A_INST = A_TILE / (1024 * NW), B_INST = B_TILE / (1024 * NW);
    constexpr int NT4 = BN / WNG / 32;
    static_assert(A_INST >= 1 && B_INST >= 1 && NT4 >= 1, "tile too small for this many waves");
    constexpr int BROWB = BN * 2;            // bytes per gathered fc2^T row slice
    constexpr int BCPR = BN / 8;             // 16-byte chunks per row
    constexpr int BRPI = 1024 / BROWB;       // rows per DMA instruction (2 for BN=256, 4 for BN=128)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w / WNG, wn = w % WNG;

    // all column tiles of fc2^T are live (N2 is dense); the map only reorders them for L2 reuse (see map_tile)
    const int Gs = (p.M + BM - 1) / BM;   // groups of one sequence
    int G = Gs;
    if constexpr (BATCHED) G = Gs * p.B;
    const int xcdq = (G * p.NT) >> 3, xcdr = (G * p.NT) & 7;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    if (slot >= xcdq + (xcd < xcdr ? 1 : 0)) return;
    const int NR = p.NR;
    const int mine = xcdq + (xcd < xcdr ? 1 : 0);
    const int tbase = xcd < xcdr ? xcd * (xcdq + 1) : xcdr * (xcdq + 1) + (xcd - xcdr) * xcdq;
    auto group_of = [&](int tt) {
        const int nb_ = tt / (G * NR), rem_ = tt - nb_ * (G * NR);
        return rem_ / min(NR, p.NT - nb_ * NR);
    };
    int t = tbase + slot;
    // Length-aware placement of a ONE-ROUND launch (round 6).  A tile's k loop is as long as its group's kept count, and a launch of
    // `mine` tiles per XCD on 2 x cus_per_xcd slots lasts as long as its slowest tile.  Workgroups reach the CUs in dispatch order
    // (tools/probes/dispatch_census.hip: local index l lands on CU l mod cus_per_xcd, so l and l + cus share a CU and the indices
    // [mine - cus, cus) have a CU to themselves -- observed, a speed heuristic only), and a workgroup alone on its CU runs ~25 % faster.
    // So this XCD's tiles are ranked by length (longest first, ties by tile order) and handed out by position: the lone positions
    // take the longest tiles, pair (l, l + cus) takes the next longest together with the shortest.  Same tiles per XCD (same L2
    // working set), same arithmetic per tile: only who computes what moves.
    const int cap = p.cus_per_xcd;
    if (cap > 0 && mine > cap && mine <= 64 && mine <= 2 * cap) {
        const int nl = 2 * cap - mine;                      // lone positions: [mine - cap, cap)
        const int want = slot < mine - cap ? nl + slot      // first member of a pair: the longest of what the lone ones left
                         : slot < cap      ? slot - (mine - cap)   // alone on its CU: the longest of all
                                           : mine - 1 - (slot - cap);   // second member (partner of slot - cap): the shortest
        const int len = lane < mine ? p.counts[group_of(tbase + lane)] : -1;
        int rank = 0;
        for (int j = 0; j < mine; ++j) {
            const int lj = __shfl(len, j);
            rank += (lj > len || (lj == len && j < lane)) ? 1 : 0;
        }
        const unsigned long long hit = __ballot(lane < mine && rank == want);
        t = tbase + (int)__builtin_ctzll(hit);
    }
    const int nb = t / (G * NR), rem = t - nb * (G * NR);
    const int nr = min(NR, p.NT - nb * NR);
    const int gi = rem / nr, nt = nb * NR + rem - gi * nr;   // gi: the group's place in the index / count lists
    const int cnt = p.counts[gi];
    // g: the group inside its sequence; seq_a / seq_c: that sequence's operands (64-bit bases; the offsets below stay per sequence)
    int g = gi, bseq = 0;
    if constexpr (BATCHED) {
        bseq = gi / Gs;
        g = gi - bseq * Gs;
    }
    auto seq_a = [&]() -> const uint16_t * {
        if constexpr (BATCHED) return p.a + (int64_t)bseq * p.M * p.F;
        else return p.a;
    };
    auto seq_c = [&]() -> uint16_t * {
        if constexpr (BATCHED) return p.c + (int64_t)bseq * p.M * p.N2;
        else return p.c;
    };
    const int n0 = nt * BN;
    const int ncols = min(BN, p.N2 - n0);  // N2 is a multiple of 8 (checked on the host)
    const int32_t *idxg = p.indices + (int64_t)gi * p.F;
    const int nkb = (cnt + BK - 1) / BK;
    if (nkb == 0) return;

    // ragged last group: `rows` of the 128 rows exist; the A pieces of the others re-read the last live row (a row of A only feeds its
    // own output row) and the epilogue neither loads nor stores their rows of C
    const int rows = min(BM, p.M - g * BM);
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(seq_a(), (uint32_t)p.M * p.F * 2u), rb = make_rsrc(p.b);
    uint32_t aoff[A_INST];  // byte offsets
#pragma unroll
    for (int i = 0; i < A_INST; ++i) {
        const int row = KT::lane_row(w * A_INST + i, lane);
        aoff[i] = ((uint32_t)(g * BM + min(row, rows - 1)) * p.F + KT::src_chunk_elems(row, lane)) * 2u;
    }
    // The gather keys of a tile are wave-uniform per DMA row, so they are fetched with SCALAR loads (lgkmcnt): the
    // vector-memory counter then only counts LDS-DMA and the counted vmcnt pipeline below stays intact.  The keys of
    // the tile issued NEXT iteration are fetched one iteration ahead so their latency hides behind the MFMAs.
    constexpr int NKEY = B_INST * BRPI;          // keys per wave per tile (8): consecutive entries of the index list
    static_assert(NKEY % 4 == 0, "a wave's keys are fetched as whole s_load_dwordx4/x8");
    int keys[NKEY];
    auto load_keys = [&](int kb) {
        // counts are multiples of 8 and so is the block start: the block is live or dead as a whole, which lets the
        // compiler fetch it with ONE wide scalar load instead of NKEY single ones
        const int base = kb * BK + w * NKEY;
        // through the CONSTANT address space: the compiler then emits s_load (lgkmcnt).  As a plain global pointer it loaded the keys with
        // a vector global_load -- on the vmcnt counter, so the use of a key one k step later drained every LDS-DMA in flight
        // (s_waitcnt vmcnt(0) in the middle of the ring: the prefetch depth of the ring was never there)
        const __attribute__((address_space(4))) int32_t *kp =
            (const __attribute__((address_space(4))) int32_t *)(idxg + __builtin_amdgcn_readfirstlane(base < cnt ? base : 0));
#pragma unroll
        for (int j = 0; j < NKEY; ++j) keys[j] = kp[j];
    };
    const int rsel = lane / BCPR;                  // which of the instruction's BRPI rows this lane stages
    auto issue = [&](int kb, int buf) {
        unsigned char *st = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < A_INST; ++i)
            if (!(p.probe & 32)) blds16(ra, aoff[i], kb * BK * 2, st + (w * A_INST + i) * 1024);   // (timing probe 32: no A pieces)
#pragma unroll
        for (int i = 0; i < B_INST; ++i) {
            if (p.probe & 64) continue;                                                        // (timing probe 64: no B pieces)
            int key = keys[i * BRPI];
#pragma unroll
            for (int rr = 1; rr < BRPI; ++rr) key = rsel == rr ? keys[i * BRPI + rr] : key;
            const int r = (w * B_INST + i) * BRPI + rsel;
            int chunk = (lane % BCPR) ^ ((r & 3) << 2);
            chunk = chunk * 8 < ncols ? chunk : 0;  // partial last column tile: stay inside the row
            blds16(rb, ((uint32_t)key * p.N2 + n0 + chunk * 8) * 2u, 0, st + A_TILE + (w * B_INST + i) * 1024);
        }
    };

    f32x16 acc[NT4][2];  // [n tile][m tile]: MFMA rows = n (fc2^T via transpose reads), MFMA cols = m
#pragma unroll
    for (int n4 = 0; n4 < NT4; ++n4)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[n4][mt][r] = 0.f;

#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
        if (s < nkb) {
            load_keys(s);
            issue(s, s);
        }
    if (NST - 1 < nkb) load_keys(NST - 1);
    const int li = lane & 15, grp = lane >> 4;
    int buf = 0, nbuf = NST - 1;
    MPROF_DECL;
    MPROF_START();
    for (int kb = 0; kb < nkb; ++kb) {
        if (kb + NST - 1 <= nkb) wait_vmcnt<(NST - 2) * (A_INST + B_INST)>();
        else wait_vmcnt<0>();
        MPROF_MARK(0);
        __builtin_amdgcn_s_barrier();
        MPROF_MARK(1);
        // An 8-wave workgroup puts waves w and w + 4 on the same SIMD, locked to each other by the barrier: both would issue their DMA
        // pieces first and want the matrix pipe afterwards.  The second wave of each SIMD issues its pieces AFTER its MFMAs instead, so
        // the pair is in complementary phases (same-box A/B, FLUX shape: 154.8 -> 148.7 us; p.probe & 8 switches it off).
        const bool late = NW == 8 && !(p.probe & 8) && w >= NW / 2;
        if (!late && kb + NST - 1 < nkb) {
            issue(kb + NST - 1, nbuf);
            if (kb + NST < nkb) load_keys(kb + NST);  // (moving these behind the MFMAs measured 15 % slower)
        }
        MPROF_MARK(2);
        // Operand fragments by inline-asm LDS reads with hand-counted lgkmcnt (EVERY LDS read of this loop has to stay in asm: one
        // compiler-visible LDS access added here later brings the drain back and is not counted by the waits below -- tests/test_kernel_audit.py
        // checks the loop's ISA for it): hipcc puts s_waitcnt vmcnt(0) in front of every LDS read
        // it knows about while an LDS-DMA is in flight (it cannot tell the ring slots apart), which drained the two stages the ring is
        // meant to keep flying.  Reads return in order; a scalar key load in flight only makes a counted wait conservative.
        constexpr int KK = BK / 16;
        constexpr int RD = 2 + 2 * NT4;   // LDS reads per k slice: two A fragments, two halves per B fragment
        const uint32_t stage_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem + buf * STAGE;
        u32x4 pf[KK][2];
        u32x2 wlo[KK][NT4], whi[KK][NT4];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int row = wm * 64 + mt * 32 + (lane & 31);
                const uint32_t ad = stage_lds + row * KT::ROWB + (((kk * 2 + (lane >> 5)) ^ KT::swz(row)) << 4);
                asm volatile("ds_read_b128 %0, %1" : "=&v"(pf[kk][mt]) : "v"(ad) : "memory");
            }
#pragma unroll
            for (int n4 = 0; n4 < NT4; ++n4) {
                // lane group grp: n half = grp&1, k half = grp>>1; lane li addresses block row li>>2, cols (li&3)*4
                const int row = kk * 16 + (grp >> 1) * 8 + (li >> 2);
                const int chunk = (wn * (BN / WNG / 8) + n4 * 4 + (grp & 1) * 2 + ((li & 3) >> 1)) ^ ((row & 3) << 2);
                const uint32_t ad = stage_lds + A_TILE + row * BROWB + chunk * 16 + (li & 1) * 8;
                asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:%c3"
                             : "=&v"(wlo[kk][n4]), "=&v"(whi[kk][n4]) : "v"(ad), "i"(4 * BROWB) : "memory");   // (early clobber: a result
                // register shared with the address would be overwritten by the first read's return if the second one queues behind it)
            }
        }
        if (kb == nkb - 1) {   // packed columns past the count hold garbage: only the last k step can see them (counts are multiples of 8)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const bool kdead = kb * BK + kk * 16 + (lane >> 5) * 8 >= cnt;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    asm volatile("" : "+v"(pf[kk][mt]));
                    if (kdead) pf[kk][mt] = (u32x4){0u, 0u, 0u, 0u};
                }
            }
        }
        static_for<0, KK>([&](auto kc) {
            constexpr int kk = decltype(kc)::value;
            // slice kk has landed once at most the reads of the younger slices are outstanding; the operands pin the MFMAs below the wait
            constexpr int YOUNGER = RD * (KK - 1 - kk);   // (the counter has 4 bits: a smaller number only waits for more)
            asm volatile("s_waitcnt lgkmcnt(%c0)" ::"i"(YOUNGER > 15 ? 15 : YOUNGER) : "memory");
#pragma unroll
            for (int i = 0; i < 2; ++i) asm volatile("" : "+v"(pf[kk][i]));
#pragma unroll
            for (int i = 0; i < NT4; ++i) asm volatile("" : "+v"(wlo[kk][i]), "+v"(whi[kk][i]));
#pragma unroll
            for (int n4 = 0; n4 < NT4; ++n4) {
                const bf16x8 wfr = __builtin_bit_cast(bf16x8, (u32x4){wlo[kk][n4][0], wlo[kk][n4][1], whi[kk][n4][0], whi[kk][n4][1]});
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) acc[n4][mt] = mfma32(wfr, __builtin_bit_cast(bf16x8, pf[kk][mt]), acc[n4][mt]);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        if (late && kb + NST - 1 < nkb) {
            issue(kb + NST - 1, nbuf);
            if (kb + NST < nkb) load_keys(kb + NST);
        }
        MPROF_MARK(3);
        buf = buf + 1 == NST ? 0 : buf + 1;
        nbuf = nbuf + 1 == NST ? 0 : nbuf + 1;
    }
    MPROF_END(w, nkb);

    if (p.probe == 4) {  // timing probe: no epilogue
        float t = 0.f;
#pragma unroll
        for (int n4 = 0; n4 < NT4; ++n4)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) t += acc[n4][mt][r];
        if (t == 123.456f) p.c[0] = 1;
        return;
    }
    // ---- epilogue: lane owns row m = lane&31 of each tile and 4 consecutive n per accumulator quad
    //      C = bf16(acc) + C in bf16  (triton/csp_mlp_mm2.py:100-101)
    constexpr bool STAGED = BM * BN * 2 <= NST * STAGE;
    if constexpr (STAGED) {
        // bf16(acc) goes through the (now free) ring as a row-major [128][BN] tile, 16-byte chunk c of row m stored at
        // chunk c ^ (m & 31) (the 32 lanes of a store hit 32 rows at one column offset); the read-modify-write of C
        // then runs as 16-byte accesses over whole BN*2-byte row segments instead of 8-byte accesses 32 rows apart.
        constexpr int CPRO = BN / 8;  // 16-byte chunks per output row
        __syncthreads();              // every wave is done reading the last operand stage
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int ml = wm * 64 + mt * 32 + (lane & 31);
#pragma unroll
            for (int n4 = 0; n4 < NT4; ++n4) {
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const int nl = wn * (BN / WNG) + n4 * 32 + q4 * 8 + (lane >> 5) * 4;
                    u32x2 v;
                    v[0] = pack_bf16x2(acc[n4][mt][q4 * 4 + 0], acc[n4][mt][q4 * 4 + 1]);
                    v[1] = pack_bf16x2(acc[n4][mt][q4 * 4 + 2], acc[n4][mt][q4 * 4 + 3]);
                    *(u32x2 *)(smem + ml * (BN * 2) + ((((nl >> 3) ^ (ml & (CPRO - 1) & 31)) << 4) | ((nl & 4) << 1))) = v;
                }
            }
        }
        __syncthreads();
        constexpr int ITEMS = BM * CPRO / (NW * 64);  // 16-byte pieces per thread
        // all of the thread's C pieces are requested before the first is used: written as load -> add -> store per piece, every load
        // sits behind the previous piece's store (same array, may alias) and hipcc drains both with vmcnt(0) -- eight serial HBM round
        // trips at the end of every tile, and the tiles of a launch all end together
        u32x4 olds[ITEMS];
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int item = it * (NW * 64) + tid;
            const int r = item / CPRO, ch = item % CPRO;
            const int n = n0 + ch * 8;
            olds[it] = (n < p.N2 && r < rows) ? *(const u32x4 *)(seq_c() + (int64_t)(g * BM + r) * p.N2 + n) : (u32x4){0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int item = it * (NW * 64) + tid;
            const int r = item / CPRO, ch = item % CPRO;
            const int n = n0 + ch * 8;
            if (n >= p.N2 || r >= rows) continue;  // N2 is a multiple of 8: a chunk is live or dead as a whole
            const u32x4 a = *(const u32x4 *)(smem + r * (BN * 2) + ((ch ^ (r & (CPRO - 1) & 31)) << 4));
            uint16_t *cp = seq_c() + (int64_t)(g * BM + r) * p.N2 + n;
            const u32x4 old = olds[it];
            u32x4 out;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                out[e] = pack_bf16x2(__uint_as_float(a[e] << 16) + __uint_as_float(old[e] << 16),
                                     __uint_as_float(a[e] & 0xffff0000u) + __uint_as_float(old[e] & 0xffff0000u));
            *(u32x4 *)cp = out;
        }
    } else {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int m = g * BM + wm * 64 + mt * 32 + (lane & 31);
            uint16_t *crow = seq_c() + (int64_t)m * p.N2;
#pragma unroll
            for (int n4 = 0; n4 < NT4; ++n4) {
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const int n = n0 + wn * (BN / WNG) + n4 * 32 + q4 * 8 + (lane >> 5) * 4;
                    if (n >= p.N2) continue;
                    const u32x2 old = *(const u32x2 *)(crow + n);
                    const float a0 = round_bf16(acc[n4][mt][q4 * 4 + 0]), a1 = round_bf16(acc[n4][mt][q4 * 4 + 1]);
                    const float a2 = round_bf16(acc[n4][mt][q4 * 4 + 2]), a3 = round_bf16(acc[n4][mt][q4 * 4 + 3]);
                    u32x2 out;
                    out[0] = pack_bf16x2(a0 + __uint_as_float(old[0] << 16), a1 + __uint_as_float(old[0] & 0xffff0000u));
                    out[1] = pack_bf16x2(a2 + __uint_as_float(old[1] << 16), a3 + __uint_as_float(old[1] & 0xffff0000u));
                    *(u32x2 *)(crow + n) = out;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ mm2, e4m3 weights
// (not in the probe-forms build: its entries answer with an error there)
#ifndef CHIPMUNK_MM1_PROBES
// GEMM2 over e4m3 rows of fc2^T (weight-only fp8): C = bf16(bf16((A_packed x f(fc2^T[idx])) * scale_b) + C).  mm2_kernel's loop -- the same
// ring, keys, waits, placement, ragged rows and epilogue staging -- with three differences:
//   * a gathered row slice is BN bytes, so a B tile is half of mm2_kernel's and the freed LDS is a fourth ring stage (4 x 16 KiB = the
//     64 KiB the staged epilogue needs);
//   * ds_read_b64_tr_b16 runs over the BYTE image: one 16-bit element is the column pair (2j, 2j + 1), so lane l & 31 of a read pair
//     receives 8 k-consecutive bytes of columns 2 (l & 31) and 2 (l & 31) + 1 of a 64-column block.  v_perm_b32 separates the two columns,
//     v_cvt_scalef32_pk_bf16_fp8 with scale 1.0 widens them (exact: every e4m3 value is a bf16 value) -- two MFMA fragments, "even" and
//     "odd", whose accumulator row i is column 2 i (+ 1) of the block.  k sits where mm2_kernel puts it (lane half = k half, 8 consecutive k
//     per lane, slices in order), so the fp32 sums are mm2_kernel's on the widened weights;
//   * the epilogue interleaves the even and the odd accumulator (one lane then owns 8 consecutive columns, a whole 16-byte chunk of the
//     staged tile) and multiplies by scale_b before bf16(acc).
struct Mm2W8Params {
    const uint16_t *a;       // packed [M,F] bf16
    const uint8_t *b;        // fc2^T [F,N2] e4m3
    const float *scale_b;    // the weight's reciprocal quantisation scale (device)
    uint16_t *c;             // [M,N2] bf16, accumulated in place
    const int32_t *indices, *counts;
    int M, F, N2, NT, NR;
    int cus_per_xcd;         // as Mm2Params
};
struct Mm2W8Batch : Mm2W8Params {
    int B;
};

template <int BN, int BK, int NST, int WPS, int NW, bool BATCHED>
__global__ __launch_bounds__(NW == 8 ? 512 : 256, WPS) void mm2_w8_kernel(const typename std::conditional<BATCHED, Mm2W8Batch, Mm2W8Params>::type p) {
    static_assert(NW == 4 || NW == 8, "4 waves (2 x 2) or 8 waves (2 x 4)");
    constexpr int WNG = NW / 2;                 // waves along n; wave tile = 64 rows x BN/WNG columns
    using KT = KTile<BK>;
    constexpr int A_TILE = BM * BK * 2, B_TILE = BK * BN, STAGE = A_TILE + B_TILE;
    constexpr int A_INST = A_TILE / (1024 * NW), B_INST = B_TILE / (1024 * NW);
    constexpr int NP = BN / WNG / 64;        // 64-column blocks per wave: one transpose-read pair and two accumulator tiles each
    static_assert(A_INST >= 1 && B_INST >= 1 && NP >= 1 && BN % (WNG * 64) == 0, "tile too small for this many waves");
    static_assert(BM * BN * 2 <= NST * STAGE, "the epilogue stages the bf16 output tile in the ring");
    constexpr int BROWB = BN;                // bytes per gathered fc2^T row slice
    constexpr int BCPR = BN / 16;            // 16-byte chunks per row
    constexpr int BRPI = 1024 / BROWB;       // rows per DMA instruction (4 for BN=256)
    static_assert(BCPR == 16 && BRPI == 4, "the chunk swizzle and the key select below are written for 256-byte row slices");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w / WNG, wn = w % WNG;

    // tile map and length-aware placement: mm2_kernel's
    const int Gs = (p.M + BM - 1) / BM;
    int G = Gs;
    if constexpr (BATCHED) G = Gs * p.B;
    const int xcdq = (G * p.NT) >> 3, xcdr = (G * p.NT) & 7;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    if (slot >= xcdq + (xcd < xcdr ? 1 : 0)) return;
    const int NR = p.NR;
    const int mine = xcdq + (xcd < xcdr ? 1 : 0);
    const int tbase = xcd < xcdr ? xcd * (xcdq + 1) : xcdr * (xcdq + 1) + (xcd - xcdr) * xcdq;
    auto group_of = [&](int tt) {
        const int nb_ = tt / (G * NR), rem_ = tt - nb_ * (G * NR);
        return rem_ / min(NR, p.NT - nb_ * NR);
    };
    int t = tbase + slot;
    const int cap = p.cus_per_xcd;
    if (cap > 0 && mine > cap && mine <= 64 && mine <= 2 * cap) {
        const int nl = 2 * cap - mine;
        const int want = slot < mine - cap ? nl + slot : slot < cap ? slot - (mine - cap) : mine - 1 - (slot - cap);
        const int len = lane < mine ? p.counts[group_of(tbase + lane)] : -1;
        int rank = 0;
        for (int j = 0; j < mine; ++j) {
            const int lj = __shfl(len, j);
            rank += (lj > len || (lj == len && j < lane)) ? 1 : 0;
        }
        const unsigned long long hit = __ballot(lane < mine && rank == want);
        t = tbase + (int)__builtin_ctzll(hit);
    }
    const int nb = t / (G * NR), rem = t - nb * (G * NR);
    const int nr = min(NR, p.NT - nb * NR);
    const int gi = rem / nr, nt = nb * NR + rem - gi * nr;
    const int cnt = p.counts[gi];
    int g = gi, bseq = 0;
    if constexpr (BATCHED) {
        bseq = gi / Gs;
        g = gi - bseq * Gs;
    }
    auto seq_a = [&]() -> const uint16_t * {
        if constexpr (BATCHED) return p.a + (int64_t)bseq * p.M * p.F;
        else return p.a;
    };
    auto seq_c = [&]() -> uint16_t * {
        if constexpr (BATCHED) return p.c + (int64_t)bseq * p.M * p.N2;
        else return p.c;
    };
    const int n0 = nt * BN;
    const int ncols = min(BN, p.N2 - n0);  // N2 is a multiple of 16 (checked on the host): a 16-byte chunk is live or dead as a whole
    const int32_t *idxg = p.indices + (int64_t)gi * p.F;
    const int nkb = (cnt + BK - 1) / BK;
    if (nkb == 0) return;
    const float sb = *p.scale_b;

    const int rows = min(BM, p.M - g * BM);   // ragged last group, as mm2_kernel
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(seq_a(), (uint32_t)p.M * p.F * 2u), rb = make_rsrc(p.b, (uint32_t)p.F * p.N2);
    uint32_t aoff[A_INST];  // byte offsets
#pragma unroll
    for (int i = 0; i < A_INST; ++i) {
        const int row = KT::lane_row(w * A_INST + i, lane);
        aoff[i] = ((uint32_t)(g * BM + min(row, rows - 1)) * p.F + KT::src_chunk_elems(row, lane)) * 2u;
    }
    constexpr int NKEY = B_INST * BRPI;          // keys per wave per tile (4): consecutive entries of the index list, scalar loads
    static_assert(NKEY % 4 == 0, "a wave's keys are fetched as whole s_load_dwordx4/x8");
    int keys[NKEY];
    auto load_keys = [&](int kb) {
        // counts are multiples of 8 and the block start one of 4: the block is live or dead as a whole
        const int base = kb * BK + w * NKEY;
        const __attribute__((address_space(4))) int32_t *kp =
            (const __attribute__((address_space(4))) int32_t *)(idxg + __builtin_amdgcn_readfirstlane(base < cnt ? base : 0));
#pragma unroll
        for (int j = 0; j < NKEY; ++j) keys[j] = kp[j];
    };
    const int rsel = lane / BCPR;                  // which of the instruction's BRPI rows this lane stages
    auto issue = [&](int kb, int buf) {
        unsigned char *st = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < A_INST; ++i) blds16(ra, aoff[i], kb * BK * 2, st + (w * A_INST + i) * 1024);
#pragma unroll
        for (int i = 0; i < B_INST; ++i) {
            // (a two-level select on the bits of rsel: the chain `rsel == rr ? keys[rr] : key` over four keys is compiled into an indexed
            // load from a scratch copy of the keys)
            const int klo = (rsel & 1) ? keys[i * BRPI + 1] : keys[i * BRPI], khi = (rsel & 1) ? keys[i * BRPI + 3] : keys[i * BRPI + 2];
            const int key = (rsel & 2) ? khi : klo;
            const int r = (w * B_INST + i) * BRPI + rsel;
            int chunk = (lane % BCPR) ^ ((r & 3) << 2);
            chunk = chunk * 16 < ncols ? chunk : 0;  // partial last column tile: stay inside the row
            blds16(rb, (uint32_t)key * p.N2 + n0 + chunk * 16, 0, st + A_TILE + (w * B_INST + i) * 1024);
        }
    };

    f32x16 acc[NP][2][2];  // [64-column block][even / odd columns][m tile]: MFMA rows = n, MFMA cols = m
#pragma unroll
    for (int np = 0; np < NP; ++np)
#pragma unroll
        for (int eo = 0; eo < 2; ++eo)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[np][eo][mt][r] = 0.f;

#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
        if (s < nkb) {
            load_keys(s);
            issue(s, s);
        }
    if (NST - 1 < nkb) load_keys(NST - 1);
    const int li = lane & 15, grp = lane >> 4;
    int buf = 0, nbuf = NST - 1;
    for (int kb = 0; kb < nkb; ++kb) {
        if (kb + NST - 1 <= nkb) wait_vmcnt<(NST - 2) * (A_INST + B_INST)>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        const bool late = NW == 8 && w >= NW / 2;   // the second wave of each SIMD issues its pieces after its MFMAs (see mm2_kernel)
        if (!late && kb + NST - 1 < nkb) {
            issue(kb + NST - 1, nbuf);
            if (kb + NST < nkb) load_keys(kb + NST);
        }
        // every LDS read of the loop in inline asm with hand-counted lgkmcnt (see mm2_kernel)
        constexpr int KK = BK / 16;
        constexpr int RD = 2 + 2 * NP;   // LDS reads per k slice: two A fragments, two halves per 64-column block
        const uint32_t stage_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem + buf * STAGE;
        u32x4 pf[KK][2];
        u32x2 wlo[KK][NP], whi[KK][NP];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int row = wm * 64 + mt * 32 + (lane & 31);
                const uint32_t ad = stage_lds + row * KT::ROWB + (((kk * 2 + (lane >> 5)) ^ KT::swz(row)) << 4);
                asm volatile("ds_read_b128 %0, %1" : "=&v"(pf[kk][mt]) : "v"(ad) : "memory");
            }
#pragma unroll
            for (int np = 0; np < NP; ++np) {
                // lane group grp: column half = grp&1 (32 columns = 32 bytes), k half = grp>>1; lane li addresses block row li>>2, bytes (li&3)*8
                const int row = kk * 16 + (grp >> 1) * 8 + (li >> 2);
                const int chunk = (wn * (BN / WNG / 16) + np * 4 + (grp & 1) * 2 + ((li & 3) >> 1)) ^ ((row & 3) << 2);
                const uint32_t ad = stage_lds + A_TILE + row * BROWB + chunk * 16 + (li & 1) * 8;
                asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:%c3"
                             : "=&v"(wlo[kk][np]), "=&v"(whi[kk][np]) : "v"(ad), "i"(4 * BROWB) : "memory");
            }
        }
        if (kb == nkb - 1) {   // packed columns past the count hold garbage: only the last k step can see them (counts are multiples of 8)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const bool kdead = kb * BK + kk * 16 + (lane >> 5) * 8 >= cnt;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    asm volatile("" : "+v"(pf[kk][mt]));
                    if (kdead) pf[kk][mt] = (u32x4){0u, 0u, 0u, 0u};
                }
            }
        }
        static_for<0, KK>([&](auto kc) {
            constexpr int kk = decltype(kc)::value;
            constexpr int YOUNGER = RD * (KK - 1 - kk);
            asm volatile("s_waitcnt lgkmcnt(%c0)" ::"i"(YOUNGER > 15 ? 15 : YOUNGER) : "memory");
#pragma unroll
            for (int i = 0; i < 2; ++i) asm volatile("" : "+v"(pf[kk][i]));
#pragma unroll
            for (int i = 0; i < NP; ++i) asm volatile("" : "+v"(wlo[kk][i]), "+v"(whi[kk][i]));
#pragma unroll
            for (int np = 0; np < NP; ++np) {
                // wlo = {k0 | k1 << 16, k2 | k3 << 16}, each 16 bits = {even column, odd column}; whi: k4 .. k7
#pragma unroll
                for (int eo = 0; eo < 2; ++eo) {
                    const uint32_t sel = eo ? 0x07050301u : 0x06040200u;
                    const uint32_t k03 = __builtin_amdgcn_perm(wlo[kk][np][1], wlo[kk][np][0], sel);
                    const uint32_t k47 = __builtin_amdgcn_perm(whi[kk][np][1], whi[kk][np][0], sel);
                    const bf16x2 f0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(k03, 1.0f, false);
                    const bf16x2 f1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(k03, 1.0f, true);
                    const bf16x2 f2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(k47, 1.0f, false);
                    const bf16x2 f3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(k47, 1.0f, true);
                    const bf16x8 wfr = {f0[0], f0[1], f1[0], f1[1], f2[0], f2[1], f3[0], f3[1]};
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) acc[np][eo][mt] = mfma32(wfr, __builtin_bit_cast(bf16x8, pf[kk][mt]), acc[np][eo][mt]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        if (late && kb + NST - 1 < nkb) {
            issue(kb + NST - 1, nbuf);
            if (kb + NST < nkb) load_keys(kb + NST);
        }
        buf = buf + 1 == NST ? 0 : buf + 1;
        nbuf = nbuf + 1 == NST ? 0 : nbuf + 1;
    }

    // ---- epilogue: lane owns row m = lane&31 of each tile; accumulator register q4*4 + j is block column 2 (q4*8 + (lane>>5)*4 + j)
    //      (+ 1 in the odd tile), so j = 0..3 of both tiles are 8 consecutive columns.  C = bf16(acc * scale_b) + C in bf16, staged
    //      through the ring as in mm2_kernel (row-major [128][BN] bf16, chunk c of row m at chunk c ^ (m & 31))
    constexpr int CPRO = BN / 8;  // 16-byte chunks per output row
    __syncthreads();              // every wave is done reading the last operand stage
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int ml = wm * 64 + mt * 32 + (lane & 31);
#pragma unroll
        for (int np = 0; np < NP; ++np) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int nl = wn * (BN / WNG) + np * 64 + q4 * 16 + (lane >> 5) * 8;
                u32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = pack_bf16x2(acc[np][0][mt][q4 * 4 + j] * sb, acc[np][1][mt][q4 * 4 + j] * sb);
                *(u32x4 *)(smem + ml * (BN * 2) + (((nl >> 3) ^ (ml & (CPRO - 1) & 31)) << 4)) = v;
            }
        }
    }
    __syncthreads();
    constexpr int ITEMS = BM * CPRO / (NW * 64);  // 16-byte pieces per thread; all requested before the first is used (see mm2_kernel)
    u32x4 olds[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int item = it * (NW * 64) + tid;
        const int r = item / CPRO, ch = item % CPRO;
        const int n = n0 + ch * 8;
        olds[it] = (n < p.N2 && r < rows) ? *(const u32x4 *)(seq_c() + (int64_t)(g * BM + r) * p.N2 + n) : (u32x4){0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int item = it * (NW * 64) + tid;
        const int r = item / CPRO, ch = item % CPRO;
        const int n = n0 + ch * 8;
        if (n >= p.N2 || r >= rows) continue;  // N2 is a multiple of 16: a chunk is live or dead as a whole
        const u32x4 a = *(const u32x4 *)(smem + r * (BN * 2) + ((ch ^ (r & (CPRO - 1) & 31)) << 4));
        uint16_t *cp = seq_c() + (int64_t)(g * BM + r) * p.N2 + n;
        const u32x4 old = olds[it];
        u32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            out[e] = pack_bf16x2(__uint_as_float(a[e] << 16) + __uint_as_float(old[e] << 16),
                                 __uint_as_float(a[e] & 0xffff0000u) + __uint_as_float(old[e] & 0xffff0000u));
        *(u32x4 *)cp = out;
    }
}
#endif   // CHIPMUNK_MM1_PROBES

// ------------------------------------------------------------------------------------------------ scatter-add
// unpacked[idx[g,c], g*128 + r] += packed[g*128 + r, c]   (scatter_add.cu:43-98).  One workgroup = (group, 64 packed
// columns): the 128x64 packed tile is transposed through LDS so both the read (128 B per row) and the read-modify-write
// of the column-major cache (256 B per column) are full-line accesses.  Every (group, column) pair is owned by exactly
// one workgroup, so no atomics are needed (the reference needs TMA reduce-add only because of its thread mapping).
constexpr int SC_COLS = 64;
constexpr int SC_LD = 136;  // padded row length of the transposed tile (bf16 elements)

// Batched launch (one trailing argument: the elements between the caches of consecutive sequences): blockIdx.y walks the B * G groups
// of indices [B, G, F] / counts [B, G]; packed is [B, M, F].  The pointers move to the group's sequence, then everything is as below.
// gs: the elements between the row groups of a cache column, as Mm1Params::gs (128: column-major [F, ldc]; F * 128 with ldc = 128: group-major).
template <class... BS>
__global__ __launch_bounds__(256) void scatter_add_kernel(const uint16_t *packed, uint16_t *unpacked,
                                                          const int32_t *indices, const int32_t *counts, int M, int F, int ldc, int gs,
                                                          BS... cache_bs) {
    static_assert(sizeof...(BS) <= 1, "at most the cache batch stride");
    __shared__ __attribute__((aligned(16))) uint16_t tile[SC_COLS * SC_LD];
    if constexpr (sizeof...(BS) == 1) {
        const int Gs = (M + 127) / 128, b = blockIdx.y / Gs;
        packed += (int64_t)b * M * F, unpacked += (int64_t)b * (int64_t)(cache_bs + ...);
        indices += (int64_t)b * Gs * F, counts += b * Gs;
    }
    const int g = sizeof...(BS) == 1 ? blockIdx.y % ((M + 127) / 128) : blockIdx.y, c0 = blockIdx.x * SC_COLS;
    const int cnt = counts[g];
    if (c0 >= cnt) return;
    const int tid = threadIdx.x;
    const int rows = min(128, M - g * 128);   // ragged last group: rows past M are neither read from `packed` nor written to the cache
    // load: 128 rows x 8 chunks of 16 B
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int item = i * 256 + tid;
        const int r = item >> 3, ch = item & 7;
        const u32x4 v = r < rows ? *(const u32x4 *)(packed + (int64_t)(g * 128 + r) * F + c0 + ch * 8) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            tile[(ch * 8 + 2 * e) * SC_LD + r] = (uint16_t)(v[e] & 0xffffu);
            tile[(ch * 8 + 2 * e + 1) * SC_LD + r] = (uint16_t)(v[e] >> 16);
        }
    }
    __syncthreads();
    // accumulate: 64 columns x 16 chunks of 8 rows (the four cache pieces of a thread are requested before the first is used: a load behind the
    // previous piece's store would wait for both)
    u32x4 olds[4];
    const uint16_t *src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int item = i * 256 + tid;
        const int c = item >> 4, ch = item & 15;
        src[i] = nullptr;
        olds[i] = (u32x4){0u, 0u, 0u, 0u};
        if (c0 + c >= cnt || ch * 8 >= rows) continue;   // a piece that starts below M lies inside its column (ldc >= ceil8(M))
        const int col = indices[(int64_t)g * F + c0 + c];
        src[i] = unpacked + (int64_t)col * ldc + (int64_t)g * gs + ch * 8;
        olds[i] = *(const u32x4 *)src[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int item = i * 256 + tid;
        const int c = item >> 4, ch = item & 15;
        if (src[i] == nullptr) continue;
        const u32x4 old = olds[i];
        const u32x4 add = *(const u32x4 *)(tile + c * SC_LD + ch * 8);
        u32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            out[e] = pack_bf16x2(__uint_as_float(old[e] << 16) + __uint_as_float(add[e] << 16),
                                 __uint_as_float(old[e] & 0xffff0000u) + __uint_as_float(add[e] & 0xffff0000u));
        *(u32x4 *)const_cast<uint16_t *>(src[i]) = out;
    }
}

// ------------------------------------------------------------------------------------------------ full step: rows to row groups
// [B, R, C] -> [B, G, C, 128] for 16-bit elements, G = ceil(R / 128): the group-major activation cache of a full step, element
// (b, g, c, r) = src[b, g * 128 + r, c], the rows of the last group at or past R zero.  transpose16's 64 x 64 tiles through LDS (128-byte
// row segments on both sides); a tile lies inside one group (64 divides 128), so its 64 output rows are 128-byte halves of 256-byte
// group columns, and the tile rows past R are written as the zeros they were loaded as.
__global__ __launch_bounds__(256) void transpose16_groups_kernel(const uint16_t *src, uint16_t *dst, int R, int C) {
    __shared__ __attribute__((aligned(16))) uint16_t tile[64][72];
    const int G = (R + 127) / 128;
    const int64_t boff = (int64_t)blockIdx.z * R * C;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;   // blockIdx.y < 2 * G
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int item = i * 256 + tid, r = item >> 3, ch = item & 7;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r0 + r < R && c0 + ch * 8 + 8 <= C && (C & 7) == 0) v = *(const u32x4 *)(src + boff + (int64_t)(r0 + r) * C + c0 + ch * 8);
        else if (r0 + r < R)
            for (int e = 0; e < 8; ++e)
                if (c0 + ch * 8 + e < C) {
                    const uint32_t x = src[boff + (int64_t)(r0 + r) * C + c0 + ch * 8 + e];
                    v[e >> 1] |= x << (16 * (e & 1));
                }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            tile[ch * 8 + 2 * e][r] = (uint16_t)(v[e] & 0xffffu);
            tile[ch * 8 + 2 * e + 1][r] = (uint16_t)(v[e] >> 16);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int item = i * 256 + tid, c = item >> 3, ch = item & 7;
        if (c0 + c >= C) continue;
        // group r0 / 128, row r0 % 128 + ch * 8 of column c0 + c: 16-byte aligned, inside the [G, C, 128] block of sequence blockIdx.z
        uint16_t *d = dst + (((int64_t)blockIdx.z * G + (r0 >> 7)) * C + c0 + c) * 128 + (r0 & 127) + ch * 8;
        *(u32x4 *)d = *(const u32x4 *)&tile[c][ch * 8];
    }
}

int check_mlp_common(int M, int F, const int32_t *indices, const int32_t *counts) {
    CM_CHECK(indices && counts, "mlp: indices / counts missing");
    CM_CHECK(M > 0 && M % BM == 0, "mlp: M must be a positive multiple of 128 (got %d)", M);
    CM_CHECK(F > 0 && F % 64 == 0, "mlp: F must be a positive multiple of 64 (got %d)", F);
    return CHIPMUNK_OK;
}
// The *_ragged entries: any positive M (G = ceil(M / 128) groups, the last one short) ...
int check_mlp_ragged(int M, int F, const int32_t *indices, const int32_t *counts) {
    CM_CHECK(indices && counts, "mlp: indices / counts missing");
    CM_CHECK(M > 0, "mlp: M must be positive (got %d)", M);
    CM_CHECK(F > 0 && F % 64 == 0, "mlp: F must be a positive multiple of 64 (got %d)", F);
    return CHIPMUNK_OK;
}
// ... and a pitch for the column-major cache [F, ldc]
int check_cache_pitch(int M, int F, int ldc) {
    CM_CHECK(ldc >= M && ldc % 8 == 0,
             "mlp: the cache pitch ldc must be at least M and a multiple of 8 elements (got ldc = %d, M = %d): a [F, M] cache with M %% 8 != 0 "
             "needs padded columns", ldc, M);
    CM_CHECK((int64_t)F * ldc < (1ll << 31), "mlp: F * ldc too large for 32-bit offsets");
    return CHIPMUNK_OK;
}

// The *_batched entries: B sequences in one launch, the ragged contract per sequence
int check_mlp_batch(int B, int M) {
    CM_CHECK(B >= 1, "mlp: the batch size B must be at least 1 (got %d)", B);
    CM_CHECK((int64_t)B * ((M + BM - 1) / BM) <= 65535, "mlp: B * ceil(M / 128) groups must not exceed 65535 (got B = %d, M = %d)", B, M);
    return CHIPMUNK_OK;
}
int check_cache_batch_stride(int F, int ldc, int64_t cache_bs) {
    CM_CHECK(cache_bs >= (int64_t)F * ldc && cache_bs % 8 == 0,
             "mlp: the cache batch stride must be at least F * ldc and a multiple of 8 elements (got %lld, F * ldc = %lld)",
             (long long)cache_bs, (long long)F * ldc);
    return CHIPMUNK_OK;
}

// The *_gm entries: the group-major cache [G, F, 128] of a sequence (G = ceil(M / 128)), [B, G, F, 128] with a batch stride of its own
int check_cache_groups(int M, int F, int64_t cache_bs) {
    const int64_t block = (int64_t)((M + BM - 1) / BM) * F * BM;
    CM_CHECK(block < (1ll << 31), "mlp: G * F * 128 too large for 32-bit offsets (the group-major cache of one sequence, G = ceil(M / 128))");
    CM_CHECK(cache_bs >= block && cache_bs % 8 == 0,
             "mlp: the cache batch stride must be at least G * F * 128 and a multiple of 8 elements (got %lld, G * F * 128 = %lld)",
             (long long)cache_bs, (long long)block);
    return CHIPMUNK_OK;
}

int launch_scatter_add(const void *packed, void *unpacked, const int32_t *indices, const int32_t *counts, int M, int F, int ldc,
                       hipStream_t s, int gs = BM) {
    hipLaunchKernelGGL(scatter_add_kernel<>, dim3(F / SC_COLS, (M + BM - 1) / BM), dim3(256), 0, s, (const uint16_t *)packed,
                       (uint16_t *)unpacked, indices, counts, M, F, ldc, gs);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}
int launch_scatter_add_batched(const void *packed, void *unpacked, const int32_t *indices, const int32_t *counts, int B, int M, int F,
                               int ldc, int64_t cache_bs, hipStream_t s, int gs = BM) {
    hipLaunchKernelGGL(scatter_add_kernel<int64_t>, dim3(F / SC_COLS, B * ((M + BM - 1) / BM)), dim3(256), 0, s, (const uint16_t *)packed,
                       (uint16_t *)unpacked, indices, counts, M, F, ldc, gs, cache_bs);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

// B > 0: the batched instantiation over B * G groups
template <int BN, int BK, int NST, int WPS, int NW = 4, bool BATCHED = false>
int launch_mm2_variant(const Mm2Params &p0, hipStream_t s, int B = 1) {
    constexpr int LDS = NST * (BM * BK * 2 + BK * BN * 2);
    auto kern = mm2_kernel<BN, BK, NST, WPS, NW, BATCHED>;
    static uint64_t lds_set = 0;
    ensure_dynamic_lds((const void *)kern, LDS, lds_set);
    Mm2Params p = p0;
    p.NT = (p.N2 + BN - 1) / BN;
    p.NR = chipmunk_get_option("mm2_nr") > 0 ? chipmunk_get_option("mm2_nr") : 4;
    if (p.NR > p.NT) p.NR = p.NT;
    // length-aware placement: two-workgroups-per-CU forms only (what the census measured); option mm2_order = 1 keeps tile order
    p.cus_per_xcd = (WPS == 2 && !chipmunk_get_option("mm2_order")) ? device_cu_count() / 8 : 0;
    const dim3 grid(((B * ((p.M + BM - 1) / BM) * p.NT + 7) / 8) * 8);
    if constexpr (BATCHED) {
        Mm2Batch q;
        static_cast<Mm2Params &>(q) = p;
        q.B = B;
        hipLaunchKernelGGL(kern, grid, dim3(NW * 64), LDS, s, q);
    } else {
        hipLaunchKernelGGL(kern, grid, dim3(NW * 64), LDS, s, p);
    }
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

int launch_mm2(const void *a, const void *b, void *c, const int32_t *indices, const int32_t *counts, int M, int F, int N2,
               hipStream_t s, int B = 0) {
    CM_CHECK(N2 > 0 && N2 % 8 == 0, "mm2: N2 must be a positive multiple of 8 (got %d)", N2);
    CM_CHECK((int64_t)M * F < (1ll << 31) && (int64_t)F * N2 < (1ll << 31), "mm2: M*F or F*N2 too large for 32-bit offsets");
    Mm2Params p = {(const uint16_t *)a, (const uint16_t *)b, (uint16_t *)c, indices, counts, M, F, N2, 0, 0, chipmunk_get_option("mm1_probe")};
    if (B > 0) return launch_mm2_variant<256, 32, 3, 2, 8, true>(p, s, B);   // the *_batched entries: the shipped form only
#ifdef CHIPMUNK_MM1_PROBES
    if (M % BM == 0) switch (chipmunk_get_option("mm2_variant")) {   // (the probe forms know whole groups only)
        case 1: return launch_mm2_variant<256, 64, 2, 1>(p, s);
        case 2: return launch_mm2_variant<128, 64, 2, 2>(p, s);
        case 3: return launch_mm2_variant<128, 64, 3, 1>(p, s);
        case 5: return launch_mm2_variant<256, 64, 3, 1>(p, s);
        case 6: return launch_mm2_variant<128, 32, 4, 2>(p, s);
        case 7: return launch_mm2_variant<128, 32, 3, 3>(p, s);
        case 8: return launch_mm2_variant<256, 32, 3, 3>(p, s);
        case 9: return launch_mm2_variant<256, 64, 2, 2>(p, s);
        case 10: return launch_mm2_variant<256, 64, 3, 1, 8>(p, s);
        case 11: return launch_mm2_variant<256, 64, 2, 1, 8>(p, s);
        case 12: return launch_mm2_variant<256, 32, 3, 2, 8>(p, s);
        case 13: return launch_mm2_variant<256, 32, 4, 1, 8>(p, s);
        case 14: return launch_mm2_variant<256, 32, 3, 2>(p, s);  // the 4-wave form of the default
        case 15: return launch_mm2_variant<512, 32, 4, 2, 8>(p, s);  // 128 x 512 tiles, one workgroup per CU, wave tile 64 x 128
        case 16: return launch_mm2_variant<512, 32, 3, 2, 8>(p, s);
        default: break;
    }
#endif
    // 8 waves (2 x 4, 64 x 64 per wave, 4 waves per SIMD) x 2 workgroups per CU: equal to the 4-wave form in
    // isolation, 2 % faster inside the bench loop (A/B on one box: 170.5 -> 167.3 us, twice)
    return launch_mm2_variant<256, 32, 3, 2, 8>(p, s);
}

#ifndef CHIPMUNK_MM1_PROBES
// GEMM2 over e4m3 weights: the shipped shape of launch_mm2 with the halved B tile spent on a fourth ring stage; B > 0: the batched form
template <bool BATCHED>
int launch_mm2_w8_variant(Mm2W8Params p, hipStream_t s, int B) {
    constexpr int BN = 256, BK = 32, NST = 4, WPS = 2, NW = 8;
    constexpr int LDS = NST * (BM * BK * 2 + BK * BN);
    auto kern = mm2_w8_kernel<BN, BK, NST, WPS, NW, BATCHED>;
    static uint64_t lds_set = 0;
    ensure_dynamic_lds((const void *)kern, LDS, lds_set);
    p.NT = (p.N2 + BN - 1) / BN;
    const int nr_option = chipmunk_get_option("mm2_nr");   // column tiles per walk and placement: launch_mm2_variant's
    p.NR = nr_option > 0 ? nr_option : 4;
    if (p.NR > p.NT) p.NR = p.NT;
    p.cus_per_xcd = !chipmunk_get_option("mm2_order") ? device_cu_count() / 8 : 0;
    const dim3 grid(((B * ((p.M + BM - 1) / BM) * p.NT + 7) / 8) * 8);
    if constexpr (BATCHED) {
        Mm2W8Batch q;
        static_cast<Mm2W8Params &>(q) = p;
        q.B = B;
        hipLaunchKernelGGL(kern, grid, dim3(NW * 64), LDS, s, q);
    } else {
        hipLaunchKernelGGL(kern, grid, dim3(NW * 64), LDS, s, p);
    }
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

int launch_mm2_w8(const void *a, const void *b, const float *scale_b, void *c, const int32_t *indices, const int32_t *counts, int M, int F,
                  int N2, hipStream_t s, int B = 0) {
    CM_CHECK(a && b && scale_b && c, "csp_mlp_mm2_w8: null tensor or scale pointer");
    if (int e = check_mlp_ragged(M, F, indices, counts)) return e;
    if (B > 0) {
        if (int e = check_mlp_batch(B, M)) return e;
    }
    CM_CHECK(N2 > 0 && N2 % 16 == 0, "csp_mlp_mm2_w8: N2 must be a positive multiple of 16 (got %d): a 16-byte chunk of an e4m3 row is 16 columns", N2);
    CM_CHECK((int64_t)M * F < (1ll << 31) && (int64_t)F * N2 < (1ll << 31) && (int64_t)M * N2 < (1ll << 31),
             "csp_mlp_mm2_w8: M*F, F*N2 or M*N2 too large for 32-bit offsets");
    Mm2W8Params p = {(const uint16_t *)a, (const uint8_t *)b, scale_b, (uint16_t *)c, indices, counts, M, F, N2, 0, 0, 0};
    return B > 0 ? launch_mm2_w8_variant<true>(p, s, B) : launch_mm2_w8_variant<false>(p, s, 1);
}
#else
int launch_mm2_w8(const void *, const void *, const float *, void *, const int32_t *, const int32_t *, int, int, int, hipStream_t, int = 0) {
    CM_CHECK(false, "csp_mlp_mm2_w8: not part of the probe-forms build");
}
#endif   // CHIPMUNK_MM1_PROBES

// ACT < 0: mm1_kernel (tanh-GELU, a bias that must be there; every tile shape); ACT = CHIPMUNK_ACT_*: mm1_form_kernel
template <int BN, int BK, int NST, int WPS, bool FP8 = false, int NW = 4, bool BATCHED = false, bool GLU = false, int ACT = -1, bool RS = false>
int launch_mm1_variant(const typename Mm1Block<FP8 && GLU, false>::type &p0, hipStream_t s, bool *cache_updated = nullptr, int B = 1,
                       int64_t cache_bs = 0) {
    using P = typename Mm1Block<FP8 && GLU, false>::type;
    constexpr int PBN = GLU ? BN / 2 : BN;   // packed columns per whole tile (gated form: the B tile's rows are {gate, up} pairs)
    constexpr int STAGE = BM * BK * 2 + BN * BK * 2, LDS = NST * STAGE, EPI = BM * PBN * 2;
    // mm1_tile's staged epilogue (the one that can scatter): one stage each for cache block and outputs, or the FLAT layout
    constexpr bool STAGED = EPI <= STAGE || (NW == 8 && EPI <= (NST - 1) * STAGE && 2 * EPI <= NST * STAGE && STAGE % (BN * 2) == 0);
    auto kern = [] {
        if constexpr (ACT >= 0) return mm1_form_kernel<BN, BK, NST, WPS, FP8, GLU, ACT, RS, BATCHED>;
        else return mm1_kernel<BN, BK, NST, WPS, FP8, NW, BATCHED>;
    }();
    static_assert(ACT < 0 || NW == 4, "mm1_form_kernel has 4 waves");
    static_assert(ACT >= 0 || (!GLU && !RS), "mm1_kernel is ungated and takes scalar scales");
    static_assert(!RS || (FP8 && !GLU), "scale vectors: the ungated fp8 form only");
    static uint64_t lds_set = 0;
    ensure_dynamic_lds((const void *)kern, LDS, lds_set);
    P p = p0;
    if (!STAGED) p.update_cache = 0;
    if (cache_updated) *cache_updated = p.update_cache != 0;
    p.NT = (p.F + PBN - 1) / PBN;
    p.NR = chipmunk_get_option("mm1_nr") > 0 ? chipmunk_get_option("mm1_nr") : 4;
    if (p.NR > p.NT) p.NR = p.NT;
    // tail split: WPS workgroups per CU are resident; an XCD's leftover tiles are handed out as sub-tiles at the end of its list.  The
    // persistent grid and the split both count on WPS workgroups REALLY fitting a CU: variants whose LDS does not allow it
    // (<128,64,2,3> / <128,64,2,4>: 3-4 x 64 KiB) get the count their LDS allows -- the output is right either way, the tail balance is not
    constexpr int WPS_FIT = (160 * 1024 / LDS) < WPS ? (160 * 1024 / LDS) : WPS;
    static_assert(WPS_FIT >= 1, "a variant's ring must fit the 160 KiB of a CU");
    const int resident_per_xcd = WPS_FIT * device_cu_count() / 8;
    p.slots_per_xcd = (chipmunk_get_option("mm1_no_split") || NW != 4 || GLU) ? 0 : resident_per_xcd;   // (the gated form has no tail split)
    // persistent grid: the resident slots, or fewer when the launch has fewer tiles than slots (every tile gets its own workgroup)
    const int tiles_per_xcd = (B * ((p.M + BM - 1) / BM) * p.NT + 7) / 8;
    const int per_xcd = tiles_per_xcd < resident_per_xcd ? tiles_per_xcd : resident_per_xcd;
    if constexpr (BATCHED) {
        typename Mm1Block<FP8 && GLU, true>::type q;
        static_cast<P &>(q) = p;
        q.B = B, q.cache_bs = cache_bs;
        hipLaunchKernelGGL(kern, dim3(per_xcd * 8), dim3(NW * 64), LDS, s, q);
    } else {
        hipLaunchKernelGGL(kern, dim3(per_xcd * 8), dim3(NW * 64), LDS, s, p);
    }
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

}  // namespace

namespace {
// What every GEMM1 entry checks behind its null pointers, `who` being the entry's name in the messages.  ragged: the *_ragged entries'
// contract (any M), otherwise the reference's (M % 128 == 0); B > 0: a *_batched entry; KM: what K must be a multiple of; coded: the entry
// takes an activation code, act; upd_max: the largest update_cache (< 0: the library's own value, not checked).  The two entries of the
// reference's contract (not coded) look at K first and do not print the update_cache they refuse.  gm: a *_gm entry -- the group-major cache
// (ldc is then 128, the pitch of a column inside its group) with B >= 1 and a batch stride.
int check_mm1(const char *who, bool ragged, const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int B,
              int64_t cache_bs, int KM, bool coded, int act, int update_cache, int upd_max, bool gm = false) {
    if (int e = ragged ? check_mlp_ragged(M, F, indices, counts) : check_mlp_common(M, F, indices, counts)) return e;
    if (gm) {
        if (int e = check_cache_groups(M, F, cache_bs)) return e;
    } else {
        if (int e = check_cache_pitch(M, F, ldc)) return e;
        if (B > 0) {
            if (int e = check_cache_batch_stride(F, ldc, cache_bs)) return e;
        }
    }
    if (coded) {
        CM_CHECK(act == CHIPMUNK_ACT_GELU_TANH || act == CHIPMUNK_ACT_SILU || act == CHIPMUNK_ACT_GELU_ERF,
                 "%s: unknown activation %d (0 = gelu_tanh, 1 = silu, 2 = gelu)", who, act);
        CM_CHECK(update_cache >= 0 && update_cache <= upd_max, "%s: update_cache must be %s (got %d)", who, upd_max == 2 ? "0, 1 or 2" : "0 or 1",
                 update_cache);
    }
    CM_CHECK(K > 0 && K % KM == 0, "%s: K must be a positive multiple of %d (got %d)", who, KM, K);
    if (!coded && upd_max >= 0) CM_CHECK(update_cache >= 0 && update_cache <= upd_max, "%s: update_cache must be 0, 1 or 2", who);
    CM_CHECK((int64_t)F * K < (1ll << 31) && (int64_t)M * K < (1ll << 31) && (int64_t)F * ldc < (1ll << 31),
             "%s: operand too large for 32-bit offsets", who);
    return CHIPMUNK_OK;
}

// `ragged`: the *_ragged entries' contract (any M, cache pitch ldc); otherwise the reference's (M % 128 == 0, ldc == M)
int mm1_entry(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
              const int32_t *counts, int M, int K, int F, int ldc, bool ragged, hipStream_t stream, int update_cache, bool *cache_updated,
              int B = 0, int64_t cache_bs = 0) {   // B > 0: the *_batched entries
    CM_CHECK(a && b && c && bias && pa_cache, "csp_mlp_mm1: null tensor pointer");
    if (int e = check_mm1("csp_mlp_mm1", ragged, indices, counts, M, K, F, ldc, B, cache_bs, 64, false, 0, update_cache, -1)) return e;
    Mm1Params p = {(const uint16_t *)a, (const uint16_t *)b, (const uint16_t *)bias, (uint16_t *)pa_cache,
                   (uint16_t *)c, indices, counts, M, K, F, 0, 0, chipmunk_get_option("mm1_probe"), 0, update_cache, nullptr, nullptr, ldc};
    if (B > 0) return launch_mm1_variant<128, 64, 2, 2, false, 4, true>(p, stream, cache_updated, B, cache_bs);   // the shipped form only
#ifdef CHIPMUNK_MM1_PROBES
    if (M % BM == 0 && ldc == M) switch (chipmunk_get_option("mm1_variant")) {   // (the probe forms know whole groups and ldc == M only)
        case 1: return launch_mm1_variant<256, 64, 2, 1>(p, stream, cache_updated);
        case 3: return launch_mm1_variant<128, 64, 3, 1>(p, stream, cache_updated);
        case 4: return launch_mm1_variant<256, 32, 3, 2>(p, stream, cache_updated);
        case 5: return launch_mm1_variant<256, 64, 3, 1>(p, stream, cache_updated);
        case 6: return launch_mm1_variant<128, 32, 4, 2>(p, stream, cache_updated);
        case 7: return launch_mm1_variant<128, 32, 3, 3>(p, stream, cache_updated);
        case 8: return launch_mm1_variant<128, 64, 2, 3>(p, stream, cache_updated);
        case 9: return launch_mm1_variant<128, 64, 2, 4>(p, stream, cache_updated);
        case 10: return launch_mm1_variant<256, 64, 3, 1, false, 8>(p, stream, cache_updated);
        case 20:   // producer / consumer form (mlp_pc.h); needs two k steps
            if (K >= 128) {
                if (cache_updated) *cache_updated = update_cache != 0;
                return launch_mm1pc<false>(p, stream);
            }
            [[fallthrough]];
        case 21:   // producer / consumer form with the DMA stream running across tile boundaries (mlp_pp.h); needs six k steps
            if (K >= 384 && chipmunk_get_option("mm1_variant") == 21) {
                if (cache_updated) *cache_updated = update_cache != 0;
                return launch_mm1pp<false>(p, stream);
            }
            [[fallthrough]];
        default: break;
    }
#endif
    return launch_mm1_variant<128, 64, 2, 2>(p, stream, cache_updated);  // measured best (profiles/r01_*); the library's one GEMM1 form
}

int mm1_scatter_entry(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                      const int32_t *counts, int M, int K, int F, int ldc, bool ragged, hipStream_t stream, int B = 0, int64_t cache_bs = 0) {
    bool done = false;
    if (int e = mm1_entry(a, b, c, bias, pa_cache, indices, counts, M, K, F, ldc, ragged, stream, 1, &done, B, cache_bs)) return e;
    // tile shapes whose epilogue does not hold the cache block in LDS: the separate scatter-add kernel
    if (done) return CHIPMUNK_OK;
    if (B > 0) return launch_scatter_add_batched(c, pa_cache, indices, counts, B, M, F, ldc, cache_bs, stream);
    return launch_scatter_add(c, pa_cache, indices, counts, M, F, ldc, stream);
}

int mm1_fp8_entry(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                  const int32_t *counts, const float *scale_a, const float *scale_b, int M, int K, int F, int ldc, bool ragged,
                  int update_cache, hipStream_t stream, int B = 0, int64_t cache_bs = 0) {
    CM_CHECK(a && b && c && bias && pa_cache && scale_a && scale_b, "csp_mlp_mm1_fp8: null tensor pointer");
    if (int e = check_mm1("csp_mlp_mm1_fp8", ragged, indices, counts, M, K, F, ldc, B, cache_bs, 128, false, 0, update_cache, 2)) return e;
    // same tile machinery as the bf16 kernel (buffer-form DMA, tail split, staged epilogue); a k step is 128 fp8 values
    Mm1Params p = {(const uint16_t *)a, (const uint16_t *)b, (const uint16_t *)bias, (uint16_t *)pa_cache, (uint16_t *)c,
                   indices, counts, M, K, F, 0, 0, chipmunk_get_option("mm1_probe"), 0, update_cache == 1 ? 2 : update_cache == 2 ? 1 : 0, scale_a, scale_b, ldc};
    if (B > 0) return launch_mm1_variant<128, 64, 2, 2, true, 4, true>(p, stream, nullptr, B, cache_bs);
#ifdef CHIPMUNK_MM1_PROBES
    if (M % BM == 0 && ldc == M) {
        if (chipmunk_get_option("mm1_variant") == 10) return launch_mm1_variant<256, 64, 3, 1, true, 8>(p, stream);
        if (chipmunk_get_option("mm1_variant") == 20 && K >= 256) return launch_mm1pc<true>(p, stream);
        if (chipmunk_get_option("mm1_variant") == 21 && K >= 768) return launch_mm1pp<true>(p, stream);
    }
#endif
    return launch_mm1_variant<128, 64, 2, 2, true>(p, stream);
}

// The forms behind mm1_form_kernel -- an activation code, a nullable bias, the *_ragged / *_batched contract --, the shipped tile shape only
// (option mm1_variant is ignored): the activation code becomes the kernel's template argument here
template <bool FP8, bool GLU, bool RS, bool BATCHED>
int launch_mm1_form_b(const typename Mm1Block<FP8 && GLU, false>::type &p, int act, hipStream_t stream, int B, int64_t cache_bs) {
#ifdef CHIPMUNK_MM1_PROBES
    if constexpr (!GLU) {   // the probe-forms library does not carry the ungated forms
        CM_CHECK(false, "csp_mlp_mm1_act: not part of the probe-forms library");
        return CHIPMUNK_OK;
    } else
#endif
    switch (act) {
        case CHIPMUNK_ACT_GELU_TANH: return launch_mm1_variant<128, 64, 2, 2, FP8, 4, BATCHED, GLU, 0, RS>(p, stream, nullptr, B, cache_bs);
        case CHIPMUNK_ACT_SILU: return launch_mm1_variant<128, 64, 2, 2, FP8, 4, BATCHED, GLU, 1, RS>(p, stream, nullptr, B, cache_bs);
        default: return launch_mm1_variant<128, 64, 2, 2, FP8, 4, BATCHED, GLU, 2, RS>(p, stream, nullptr, B, cache_bs);
    }
}
// (B > 0: the *_batched entries)
template <bool FP8, bool GLU, bool RS = false>
int launch_mm1_form(const typename Mm1Block<FP8 && GLU, false>::type &p, int act, hipStream_t stream, int B, int64_t cache_bs) {
    return B > 0 ? launch_mm1_form_b<FP8, GLU, RS, true>(p, act, stream, B, cache_bs) : launch_mm1_form_b<FP8, GLU, RS, false>(p, act, stream, 1, 0);
}

// Ungated.  scale_a / scale_b null: the bf16 form (update_cache 0 / 1); both given: the e4m3 form (update_cache 0 / 1 / 2 as chipmunk_csp_mlp_mm1_fp8)
int mm1_act_entry(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices, const int32_t *counts,
                  const float *scale_a, const float *scale_b, bool fp8, int M, int K, int F, int ldc, int act, int update_cache,
                  hipStream_t stream, int B = 0, int64_t cache_bs = 0, bool rs = false, bool gm = false) {
    // B > 0: the *_batched entries; rs: the *_rs entries; gm: the *_gm entries (group-major cache, ldc = BM, B >= 1 with 1 the single-sequence launch)
    if (fp8) CM_CHECK(a && b && c && pa_cache && scale_a && scale_b, "csp_mlp_mm1_fp8_act: null tensor or scale pointer");
    else CM_CHECK(a && b && c && pa_cache, "csp_mlp_mm1_act: null tensor pointer");
    CM_CHECK(!rs || (((uintptr_t)scale_a | (uintptr_t)scale_b) & 3) == 0, "csp_mlp_mm1_fp8_act_rs: scale_a and scale_b must be 4-byte aligned");
    if (int e = check_mm1(fp8 ? "csp_mlp_mm1_fp8_act" : "csp_mlp_mm1_act", true, indices, counts, M, K, F, ldc, B, cache_bs, fp8 ? 128 : 64, true, act,
                          update_cache, fp8 ? 2 : 1, gm))
        return e;
    // the kernel's update_cache: 1 = scatter-add of the deltas, 2 (fp8) = store the new activation -- the fp8 entries' 2 and 1
    const int upd = fp8 ? (update_cache == 1 ? 2 : update_cache == 2 ? 1 : 0) : update_cache;
    Mm1Params p = {(const uint16_t *)a, (const uint16_t *)b, (const uint16_t *)bias, (uint16_t *)pa_cache,
                   (uint16_t *)c, indices, counts, M, K, F, 0, 0, 0, 0, upd, scale_a, scale_b, ldc};
    if (gm) p.gs = F * BM, B = B == 1 ? 0 : B;
    if (rs) return launch_mm1_form<true, false, true>(p, act, stream, B, cache_bs);
    return fp8 ? launch_mm1_form<true, false>(p, act, stream, B, cache_bs) : launch_mm1_form<false, false>(p, act, stream, B, cache_bs);
}

// Gated (SwiGLU / GEGLU), bf16
int mm1_glu_entry(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate, const void *bias_up, void *pa_cache,
                  const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int act, int update_cache, hipStream_t stream,
                  int B = 0, int64_t cache_bs = 0, bool gm = false) {   // B > 0: the *_batched entry; gm: the *_gm entry, as mm1_act_entry
    CM_CHECK(a && b_gate && b_up && c && pa_cache, "csp_mlp_mm1_glu: null tensor pointer");
    if (int e = check_mm1("csp_mlp_mm1_glu", true, indices, counts, M, K, F, ldc, B, cache_bs, 64, true, act, update_cache, 1, gm)) return e;
    Mm1Params p = {(const uint16_t *)a, (const uint16_t *)b_gate, (const uint16_t *)bias_gate, (uint16_t *)pa_cache,
                   (uint16_t *)c, indices, counts, M, K, F, 0, 0, 0, 0, update_cache, nullptr, nullptr, ldc};
    p.b_up = (const uint16_t *)b_up, p.bias_up = (const uint16_t *)bias_up;
    if (gm) p.gs = F * BM, B = B == 1 ? 0 : B;
    return launch_mm1_form<false, true>(p, act, stream, B, cache_bs);
}

// Gated, e4m3 a / weights (1 byte per element): K % 128 as csp_mlp_mm1_fp8, and the three reciprocal quantisation scales
int mm1_glu_fp8_entry(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate, const void *bias_up, void *pa_cache,
                      const int32_t *indices, const int32_t *counts, const float *scale_a, const float *scale_b_gate, const float *scale_b_up,
                      int M, int K, int F, int ldc, int act, int update_cache, hipStream_t stream, int B = 0, int64_t cache_bs = 0,
                      bool gm = false) {
    CM_CHECK(a && b_gate && b_up && c && pa_cache && scale_a && scale_b_gate && scale_b_up, "csp_mlp_mm1_glu_fp8: null tensor or scale pointer");
    if (int e = check_mm1("csp_mlp_mm1_glu_fp8", true, indices, counts, M, K, F, ldc, B, cache_bs, 128, true, act, update_cache, 1, gm)) return e;
    Mm1GluF8Params p;
    static_cast<Mm1Params &>(p) = {(const uint16_t *)a, (const uint16_t *)b_gate, (const uint16_t *)bias_gate, (uint16_t *)pa_cache,
                                   (uint16_t *)c, indices, counts, M, K, F, 0, 0, 0, 0, update_cache, nullptr, nullptr, ldc};
    p.b_up = (const uint16_t *)b_up, p.bias_up = (const uint16_t *)bias_up;
    p.scale_x = scale_a, p.scale_gate = scale_b_gate, p.scale_up = scale_b_up;
    if (gm) p.gs = F * BM, B = B == 1 ? 0 : B;
    return launch_mm1_form<true, true>(p, act, stream, B, cache_bs);
}

// Weight-only e4m3 fc1: mm1_w8_kernel at its one tile shape -- <128 columns, k step 64, 3 stages, 2 workgroups per CU> --, grid and tail
// split as launch_mm1_variant sets them for the ungated forms
#ifndef CHIPMUNK_MM1_PROBES
template <int ACT, bool BATCHED>
int launch_mm1_w8_kernel(Mm1W8Params p, hipStream_t s, int B, int64_t cache_bs) {
    constexpr int BN = 128, BK = 64, NST = 3, WPS = 2;
    constexpr int LDS = NST * (BM * BK * 2 + BN * BK + BN / 32 * 16);
    static_assert(LDS <= 80 * 1024, "two workgroups share a CU's 160 KiB");
    auto kern = mm1_w8_kernel<BN, BK, NST, WPS, ACT, BATCHED>;
    static uint64_t lds_set = 0;
    ensure_dynamic_lds((const void *)kern, LDS, lds_set);
    p.NT = (p.F + BN - 1) / BN;
    const int nr_option = chipmunk_get_option("mm1_nr");   // column tiles per walk: launch_mm1_variant's
    p.NR = nr_option > 0 ? nr_option : 4;
    if (p.NR > p.NT) p.NR = p.NT;
    const int resident_per_xcd = WPS * device_cu_count() / 8;
    p.slots_per_xcd = chipmunk_get_option("mm1_no_split") ? 0 : resident_per_xcd;
    const int tiles_per_xcd = (B * ((p.M + BM - 1) / BM) * p.NT + 7) / 8;
    const int per_xcd = tiles_per_xcd < resident_per_xcd ? tiles_per_xcd : resident_per_xcd;
    if constexpr (BATCHED) {
        Mm1W8Batch q;
        static_cast<Mm1W8Params &>(q) = p;
        q.B = B, q.cache_bs = cache_bs;
        hipLaunchKernelGGL(kern, dim3(per_xcd * 8), dim3(256), LDS, s, q);
    } else {
        hipLaunchKernelGGL(kern, dim3(per_xcd * 8), dim3(256), LDS, s, p);
    }
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}
template <bool BATCHED>
int launch_mm1_w8(const Mm1W8Params &p, int act, hipStream_t s, int B, int64_t cache_bs) {
    switch (act) {
        case CHIPMUNK_ACT_GELU_TANH: return launch_mm1_w8_kernel<0, BATCHED>(p, s, B, cache_bs);
        case CHIPMUNK_ACT_SILU: return launch_mm1_w8_kernel<1, BATCHED>(p, s, B, cache_bs);
        default: return launch_mm1_w8_kernel<2, BATCHED>(p, s, B, cache_bs);
    }
}
#endif

// B > 0: the *_batched entry; gm: the *_gm entry (group-major cache, ldc = BM, B >= 1 with 1 the single-sequence launch)
int mm1_w8_entry(const void *a, const void *b, const float *scale_b, int scale_n, void *c, const void *bias, void *pa_cache,
                 const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int act, int update_cache, hipStream_t stream,
                 int B = 0, int64_t cache_bs = 0, bool gm = false) {
#ifdef CHIPMUNK_MM1_PROBES
    CM_CHECK(false, "csp_mlp_mm1_w8: not part of the probe-forms build");
#else
    CM_CHECK(a && b && scale_b && c && pa_cache, "csp_mlp_mm1_w8: null tensor or scale pointer");
    CM_CHECK(scale_n == 1 || scale_n == F, "csp_mlp_mm1_w8: scale_n must be 1 (one reciprocal scale) or F = %d (one per fc1 row), got %d", F, scale_n);
    CM_CHECK(((uintptr_t)scale_b & 3) == 0, "csp_mlp_mm1_w8: scale_b must be 4-byte aligned");
    if (int e = check_mm1("csp_mlp_mm1_w8", true, indices, counts, M, K, F, ldc, B, cache_bs, 64, true, act, update_cache, 1, gm)) return e;
    Mm1W8Params p;
    static_cast<Mm1Params &>(p) = {(const uint16_t *)a, (const uint16_t *)b, (const uint16_t *)bias, (uint16_t *)pa_cache,
                                   (uint16_t *)c, indices, counts, M, K, F, 0, 0, 0, 0, update_cache, nullptr, nullptr, ldc};
    p.scale_b = scale_b, p.scale_n = scale_n;
    if (gm) p.gs = F * BM, B = B == 1 ? 0 : B;
    return B > 0 ? launch_mm1_w8<true>(p, act, stream, B, cache_bs) : launch_mm1_w8<false>(p, act, stream, 1, 0);
#endif
}

// Gated weight-only e4m3 gate / up: mm1_glu_w8_kernel at its one tile shape -- <128 B rows = 64 packed columns, k step 64, 3 stages, 2 workgroups
// per CU> --, the grid as launch_mm1_variant sets it for the gated forms (no tail split)
#ifndef CHIPMUNK_MM1_PROBES
template <int ACT, bool BATCHED>
int launch_mm1_glu_w8_kernel(Mm1GluW8Params p, hipStream_t s, int B, int64_t cache_bs) {
    constexpr int BN = 128, BK = 64, NST = 3, WPS = 2;
    constexpr int PBN = BN / 2;   // packed columns per whole tile
    constexpr int LDS = NST * (BM * BK * 2 + BN * BK + BN / 32 * 16);
    static_assert(LDS <= 80 * 1024, "two workgroups share a CU's 160 KiB");
    static_assert(BM * PBN * 2 <= LDS / NST, "the staged epilogue: cache block and output image fit one stage each");
    auto kern = mm1_glu_w8_kernel<BN, BK, NST, WPS, ACT, BATCHED>;
    static uint64_t lds_set = 0;
    ensure_dynamic_lds((const void *)kern, LDS, lds_set);
    p.NT = (p.F + PBN - 1) / PBN;
    const int nr_option = chipmunk_get_option("mm1_nr");   // column tiles per walk: launch_mm1_variant's
    p.NR = nr_option > 0 ? nr_option : 4;
    if (p.NR > p.NT) p.NR = p.NT;
    p.slots_per_xcd = 0;   // (the gated form has no tail split)
    const int resident_per_xcd = WPS * device_cu_count() / 8;
    const int tiles_per_xcd = (B * ((p.M + BM - 1) / BM) * p.NT + 7) / 8;
    const int per_xcd = tiles_per_xcd < resident_per_xcd ? tiles_per_xcd : resident_per_xcd;
    if constexpr (BATCHED) {
        Mm1GluW8Batch q;
        static_cast<Mm1GluW8Params &>(q) = p;
        q.B = B, q.cache_bs = cache_bs;
        hipLaunchKernelGGL(kern, dim3(per_xcd * 8), dim3(256), LDS, s, q);
    } else {
        hipLaunchKernelGGL(kern, dim3(per_xcd * 8), dim3(256), LDS, s, p);
    }
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}
template <bool BATCHED>
int launch_mm1_glu_w8(const Mm1GluW8Params &p, int act, hipStream_t s, int B, int64_t cache_bs) {
    switch (act) {
        case CHIPMUNK_ACT_GELU_TANH: return launch_mm1_glu_w8_kernel<0, BATCHED>(p, s, B, cache_bs);
        case CHIPMUNK_ACT_SILU: return launch_mm1_glu_w8_kernel<1, BATCHED>(p, s, B, cache_bs);
        default: return launch_mm1_glu_w8_kernel<2, BATCHED>(p, s, B, cache_bs);
    }
}
#endif

// B > 0: the *_batched entry; gm: the *_gm entry, as mm1_w8_entry
int mm1_glu_w8_entry(const void *a, const void *b_gate, const void *b_up, const float *scale_gate, int scale_gate_n, const float *scale_up,
                     int scale_up_n, void *c, const void *bias_gate, const void *bias_up, void *pa_cache, const int32_t *indices,
                     const int32_t *counts, int M, int K, int F, int ldc, int act, int update_cache, hipStream_t stream, int B = 0,
                     int64_t cache_bs = 0, bool gm = false) {
#ifdef CHIPMUNK_MM1_PROBES
    CM_CHECK(false, "csp_mlp_mm1_glu_w8: not part of the probe-forms build");
#else
    CM_CHECK(a && b_gate && b_up && scale_gate && scale_up && c && pa_cache, "csp_mlp_mm1_glu_w8: null tensor or scale pointer");
    CM_CHECK(scale_gate_n == 1 || scale_gate_n == F,
             "csp_mlp_mm1_glu_w8: scale_gate_n must be 1 (one reciprocal scale) or F = %d (one per gate row), got %d", F, scale_gate_n);
    CM_CHECK(scale_up_n == 1 || scale_up_n == F,
             "csp_mlp_mm1_glu_w8: scale_up_n must be 1 (one reciprocal scale) or F = %d (one per up row), got %d", F, scale_up_n);
    CM_CHECK((((uintptr_t)scale_gate | (uintptr_t)scale_up) & 3) == 0, "csp_mlp_mm1_glu_w8: scale_gate and scale_up must be 4-byte aligned");
    if (int e = check_mm1("csp_mlp_mm1_glu_w8", true, indices, counts, M, K, F, ldc, B, cache_bs, 64, true, act, update_cache, 1, gm)) return e;
    Mm1GluW8Params p;
    static_cast<Mm1Params &>(p) = {(const uint16_t *)a, (const uint16_t *)b_gate, (const uint16_t *)bias_gate, (uint16_t *)pa_cache,
                                   (uint16_t *)c, indices, counts, M, K, F, 0, 0, 0, 0, update_cache, nullptr, nullptr, ldc};
    p.b_up = (const uint16_t *)b_up, p.bias_up = (const uint16_t *)bias_up;
    p.scale_gate = scale_gate, p.scale_up = scale_up, p.scale_gate_n = scale_gate_n, p.scale_up_n = scale_up_n;
    if (gm) p.gs = F * BM, B = B == 1 ? 0 : B;
    return B > 0 ? launch_mm1_glu_w8<true>(p, act, stream, B, cache_bs) : launch_mm1_glu_w8<false>(p, act, stream, 1, 0);
#endif
}
}  // namespace

// ---- gated weight-only e4m3 gate / up (include/chipmunk_hip.h, "gated fp8, weight-only")
extern "C" int chipmunk_csp_mlp_mm1_glu_w8(const void *a, const void *b_gate, const void *b_up, const float *scale_gate, int scale_gate_n,
                                           const float *scale_up, int scale_up_n, void *c, const void *bias_gate, const void *bias_up,
                                           void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int act,
                                           int update_cache, void *stream) {
    return mm1_glu_w8_entry(a, b_gate, b_up, scale_gate, scale_gate_n, scale_up, scale_up_n, c, bias_gate, bias_up, pa_cache, indices, counts, M,
                            K, F, ldc, act, update_cache, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm1_glu_w8_batched(const void *a, const void *b_gate, const void *b_up, const float *scale_gate,
                                                   int scale_gate_n, const float *scale_up, int scale_up_n, void *c, const void *bias_gate,
                                                   const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts, int M,
                                                   int K, int F, int ldc, int act, int update_cache, int B, int64_t cache_batch_stride,
                                                   void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_glu_w8_entry(a, b_gate, b_up, scale_gate, scale_gate_n, scale_up, scale_up_n, c, bias_gate, bias_up, pa_cache, indices, counts, M,
                            K, F, ldc, act, update_cache, (hipStream_t)stream, B, cache_batch_stride);
}
extern "C" int chipmunk_csp_mlp_mm1_glu_w8_gm(const void *a, const void *b_gate, const void *b_up, const float *scale_gate, int scale_gate_n,
                                              const float *scale_up, int scale_up_n, void *c, const void *bias_gate, const void *bias_up,
                                              void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K, int F, int act,
                                              int update_cache, int B, int64_t cache_batch_stride, void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_glu_w8_entry(a, b_gate, b_up, scale_gate, scale_gate_n, scale_up, scale_up_n, c, bias_gate, bias_up, pa_cache, indices, counts, M,
                            K, F, BM, act, update_cache, (hipStream_t)stream, B, cache_batch_stride, true);
}

// ---- weight-only e4m3 fc1 (include/chipmunk_hip.h, "fp8 fc1, weight-only")
extern "C" int chipmunk_csp_mlp_mm1_w8(const void *a, const void *b, const float *scale_b, int scale_n, void *c, const void *bias,
                                       void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int act,
                                       int update_cache, void *stream) {
    return mm1_w8_entry(a, b, scale_b, scale_n, c, bias, pa_cache, indices, counts, M, K, F, ldc, act, update_cache, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm1_w8_batched(const void *a, const void *b, const float *scale_b, int scale_n, void *c, const void *bias,
                                               void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc,
                                               int act, int update_cache, int B, int64_t cache_batch_stride, void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_w8_entry(a, b, scale_b, scale_n, c, bias, pa_cache, indices, counts, M, K, F, ldc, act, update_cache, (hipStream_t)stream, B,
                        cache_batch_stride);
}
extern "C" int chipmunk_csp_mlp_mm1_w8_gm(const void *a, const void *b, const float *scale_b, int scale_n, void *c, const void *bias,
                                          void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K, int F, int act,
                                          int update_cache, int B, int64_t cache_batch_stride, void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_w8_entry(a, b, scale_b, scale_n, c, bias, pa_cache, indices, counts, M, K, F, BM, act, update_cache, (hipStream_t)stream, B,
                        cache_batch_stride, true);
}

extern "C" int chipmunk_csp_mlp_mm1_glu_fp8(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                                            const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts,
                                            const float *scale_a, const float *scale_b_gate, const float *scale_b_up, int M, int K, int F,
                                            int ldc, int act, int update_cache, void *stream) {
    return mm1_glu_fp8_entry(a, b_gate, b_up, c, bias_gate, bias_up, pa_cache, indices, counts, scale_a, scale_b_gate, scale_b_up, M, K, F, ldc,
                             act, update_cache, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm1_glu_fp8_batched(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                                                    const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts,
                                                    const float *scale_a, const float *scale_b_gate, const float *scale_b_up, int M, int K,
                                                    int F, int ldc, int act, int update_cache, int B, int64_t cache_batch_stride,
                                                    void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_glu_fp8_entry(a, b_gate, b_up, c, bias_gate, bias_up, pa_cache, indices, counts, scale_a, scale_b_gate, scale_b_up, M, K, F, ldc,
                             act, update_cache, (hipStream_t)stream, B, cache_batch_stride);
}

extern "C" int chipmunk_csp_mlp_mm1_glu(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                                        const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K,
                                        int F, int ldc, int act, int update_cache, void *stream) {
    return mm1_glu_entry(a, b_gate, b_up, c, bias_gate, bias_up, pa_cache, indices, counts, M, K, F, ldc, act, update_cache, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm1_glu_batched(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                                                const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts, int M,
                                                int K, int F, int ldc, int act, int update_cache, int B, int64_t cache_batch_stride,
                                                void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_glu_entry(a, b_gate, b_up, c, bias_gate, bias_up, pa_cache, indices, counts, M, K, F, ldc, act, update_cache,
                         (hipStream_t)stream, B, cache_batch_stride);
}

// ---- ungated GEMM1 with an activation code and a nullable bias (include/chipmunk_hip.h, "Ungated activations")
extern "C" int chipmunk_csp_mlp_mm1_act(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                                        const int32_t *counts, int M, int K, int F, int ldc, int act, int update_cache, void *stream) {
    return mm1_act_entry(a, b, c, bias, pa_cache, indices, counts, nullptr, nullptr, false, M, K, F, ldc, act, update_cache, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm1_act_batched(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                                const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int act,
                                                int update_cache, int B, int64_t cache_batch_stride, void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_act_entry(a, b, c, bias, pa_cache, indices, counts, nullptr, nullptr, false, M, K, F, ldc, act, update_cache, (hipStream_t)stream,
                         B, cache_batch_stride);
}
extern "C" int chipmunk_csp_mlp_mm1_fp8_act(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                                            const int32_t *counts, const float *scale_a, const float *scale_b, int M, int K, int F, int ldc,
                                            int act, int update_cache, void *stream) {
    return mm1_act_entry(a, b, c, bias, pa_cache, indices, counts, scale_a, scale_b, true, M, K, F, ldc, act, update_cache, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm1_fp8_act_batched(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                                    const int32_t *indices, const int32_t *counts, const float *scale_a, const float *scale_b,
                                                    int M, int K, int F, int ldc, int act, int update_cache, int B,
                                                    int64_t cache_batch_stride, void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_act_entry(a, b, c, bias, pa_cache, indices, counts, scale_a, scale_b, true, M, K, F, ldc, act, update_cache, (hipStream_t)stream,
                         B, cache_batch_stride);
}

extern "C" int chipmunk_csp_mlp_mm1_fp8_act_rs(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                                               const int32_t *counts, const float *scale_a, const float *scale_b, int M, int K, int F, int ldc,
                                               int act, int update_cache, void *stream) {
    return mm1_act_entry(a, b, c, bias, pa_cache, indices, counts, scale_a, scale_b, true, M, K, F, ldc, act, update_cache, (hipStream_t)stream,
                         0, 0, true);
}
extern "C" int chipmunk_csp_mlp_mm1_fp8_act_rs_batched(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                                       const int32_t *indices, const int32_t *counts, const float *scale_a, const float *scale_b,
                                                       int M, int K, int F, int ldc, int act, int update_cache, int B,
                                                       int64_t cache_batch_stride, void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_act_entry(a, b, c, bias, pa_cache, indices, counts, scale_a, scale_b, true, M, K, F, ldc, act, update_cache, (hipStream_t)stream,
                         B, cache_batch_stride, true);
}

extern "C" int chipmunk_csp_mlp_mm1(const void *a, const void *b, void *c, const void *bias, const void *pa_cache,
                                    const int32_t *indices, const int32_t *counts, int M, int K, int F, void *stream) {
    return mm1_entry(a, b, c, bias, const_cast<void *>(pa_cache), indices, counts, M, K, F, M, false, (hipStream_t)stream, 0, nullptr);
}
extern "C" int chipmunk_csp_mlp_mm1_ragged(const void *a, const void *b, void *c, const void *bias, const void *pa_cache,
                                           const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, void *stream) {
    return mm1_entry(a, b, c, bias, const_cast<void *>(pa_cache), indices, counts, M, K, F, ldc, true, (hipStream_t)stream, 0, nullptr);
}

extern "C" int chipmunk_csp_mlp_mm1_scatter(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                            const int32_t *indices, const int32_t *counts, int M, int K, int F,
                                            void *stream) {
    return mm1_scatter_entry(a, b, c, bias, pa_cache, indices, counts, M, K, F, M, false, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm1_scatter_ragged(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                                   const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc,
                                                   void *stream) {
    return mm1_scatter_entry(a, b, c, bias, pa_cache, indices, counts, M, K, F, ldc, true, (hipStream_t)stream);
}

extern "C" int chipmunk_csp_scatter_add(const void *packed, void *unpacked_colmajor, const int32_t *indices,
                                        const int32_t *counts, int M, int F, int num_sms, void *stream) {
    (void)num_sms;
    CM_CHECK(packed && unpacked_colmajor, "csp_scatter_add: null tensor pointer");
    if (int e = check_mlp_common(M, F, indices, counts)) return e;
    return launch_scatter_add(packed, unpacked_colmajor, indices, counts, M, F, M, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_scatter_add_ragged(const void *packed, void *unpacked_colmajor, const int32_t *indices,
                                               const int32_t *counts, int M, int F, int ldc, void *stream) {
    CM_CHECK(packed && unpacked_colmajor, "csp_scatter_add: null tensor pointer");
    if (int e = check_mlp_ragged(M, F, indices, counts)) return e;
    if (int e = check_cache_pitch(M, F, ldc)) return e;
    return launch_scatter_add(packed, unpacked_colmajor, indices, counts, M, F, ldc, (hipStream_t)stream);
}

extern "C" int chipmunk_csp_mlp_mm2(const void *mma_a, const void *mma_b, void *mma_c, const int32_t *indices,
                                    const int32_t *counts, int M, int F, int N2, void *stream) {
    CM_CHECK(mma_a && mma_b && mma_c, "csp_mlp_mm2: null tensor pointer");
    if (int e = check_mlp_common(M, F, indices, counts)) return e;
    return launch_mm2(mma_a, mma_b, mma_c, indices, counts, M, F, N2, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm2_ragged(const void *mma_a, const void *mma_b, void *mma_c, const int32_t *indices,
                                           const int32_t *counts, int M, int F, int N2, void *stream) {
    CM_CHECK(mma_a && mma_b && mma_c, "csp_mlp_mm2: null tensor pointer");
    if (int e = check_mlp_ragged(M, F, indices, counts)) return e;
    return launch_mm2(mma_a, mma_b, mma_c, indices, counts, M, F, N2, (hipStream_t)stream);
}

extern "C" int chipmunk_csp_mlp_mm2_and_scatter_add(const void *packed, void *unpacked_colmajor,
                                                    const int32_t *indices, const int32_t *counts, const void *mma_a,
                                                    const void *mma_b, void *mma_c, int M, int F, int N2,
                                                    int num_sms_scatter_add, void *stream) {
    (void)num_sms_scatter_add;
    CM_CHECK(packed && unpacked_colmajor && mma_a && mma_b && mma_c, "csp_mlp_mm2_and_scatter_add: null tensor pointer");
    if (int e = check_mlp_common(M, F, indices, counts)) return e;
    if (int e = launch_scatter_add(packed, unpacked_colmajor, indices, counts, M, F, M, (hipStream_t)stream)) return e;
    return launch_mm2(mma_a, mma_b, mma_c, indices, counts, M, F, N2, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm2_and_scatter_add_ragged(const void *packed, void *unpacked_colmajor,
                                                           const int32_t *indices, const int32_t *counts, const void *mma_a,
                                                           const void *mma_b, void *mma_c, int M, int F, int N2, int ldc,
                                                           void *stream) {
    CM_CHECK(packed && unpacked_colmajor && mma_a && mma_b && mma_c, "csp_mlp_mm2_and_scatter_add: null tensor pointer");
    if (int e = check_mlp_ragged(M, F, indices, counts)) return e;
    if (int e = check_cache_pitch(M, F, ldc)) return e;
    CM_CHECK(N2 > 0 && N2 % 8 == 0, "mm2: N2 must be a positive multiple of 8 (got %d)", N2);   // before the first kernel is enqueued
    if (int e = launch_scatter_add(packed, unpacked_colmajor, indices, counts, M, F, ldc, (hipStream_t)stream)) return e;
    return launch_mm2(mma_a, mma_b, mma_c, indices, counts, M, F, N2, (hipStream_t)stream);
}

extern "C" int chipmunk_csp_mlp_mm1_fp8(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                        const int32_t *indices, const int32_t *counts, const float *scale_a,
                                        const float *scale_b, int M, int K, int F, int update_cache, void *stream) {
    return mm1_fp8_entry(a, b, c, bias, pa_cache, indices, counts, scale_a, scale_b, M, K, F, M, false, update_cache, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm1_fp8_ragged(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                               const int32_t *indices, const int32_t *counts, const float *scale_a,
                                               const float *scale_b, int M, int K, int F, int ldc, int update_cache, void *stream) {
    return mm1_fp8_entry(a, b, c, bias, pa_cache, indices, counts, scale_a, scale_b, M, K, F, ldc, true, update_cache, (hipStream_t)stream);
}

// ---- B sequences in one launch (include/chipmunk_hip.h, "Batches")
extern "C" int chipmunk_csp_mlp_mm1_batched(const void *a, const void *b, void *c, const void *bias, const void *pa_cache,
                                            const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int B,
                                            int64_t cache_batch_stride, void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_entry(a, b, c, bias, const_cast<void *>(pa_cache), indices, counts, M, K, F, ldc, true, (hipStream_t)stream, 0, nullptr, B,
                     cache_batch_stride);
}
extern "C" int chipmunk_csp_mlp_mm1_scatter_batched(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                                    const int32_t *indices, const int32_t *counts, int M, int K, int F, int ldc, int B,
                                                    int64_t cache_batch_stride, void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_scatter_entry(a, b, c, bias, pa_cache, indices, counts, M, K, F, ldc, true, (hipStream_t)stream, B, cache_batch_stride);
}
extern "C" int chipmunk_csp_mlp_mm1_fp8_batched(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                                const int32_t *indices, const int32_t *counts, const float *scale_a, const float *scale_b,
                                                int M, int K, int F, int ldc, int update_cache, int B, int64_t cache_batch_stride,
                                                void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_fp8_entry(a, b, c, bias, pa_cache, indices, counts, scale_a, scale_b, M, K, F, ldc, true, update_cache, (hipStream_t)stream, B,
                         cache_batch_stride);
}
extern "C" int chipmunk_csp_mlp_mm2_batched(const void *mma_a, const void *mma_b, void *mma_c, const int32_t *indices,
                                            const int32_t *counts, int M, int F, int N2, int B, void *stream) {
    CM_CHECK(mma_a && mma_b && mma_c, "csp_mlp_mm2: null tensor pointer");
    if (int e = check_mlp_ragged(M, F, indices, counts)) return e;
    if (int e = check_mlp_batch(B, M)) return e;
    return launch_mm2(mma_a, mma_b, mma_c, indices, counts, M, F, N2, (hipStream_t)stream, B);
}
extern "C" int chipmunk_csp_scatter_add_batched(const void *packed, void *unpacked_colmajor, const int32_t *indices,
                                                const int32_t *counts, int M, int F, int ldc, int B, int64_t cache_batch_stride,
                                                void *stream) {
    CM_CHECK(packed && unpacked_colmajor, "csp_scatter_add: null tensor pointer");
    if (int e = check_mlp_ragged(M, F, indices, counts)) return e;
    if (int e = check_mlp_batch(B, M)) return e;
    if (int e = check_cache_pitch(M, F, ldc)) return e;
    if (int e = check_cache_batch_stride(F, ldc, cache_batch_stride)) return e;
    return launch_scatter_add_batched(packed, unpacked_colmajor, indices, counts, B, M, F, ldc, cache_batch_stride, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm2_and_scatter_add_batched(const void *packed, void *unpacked_colmajor, const int32_t *indices,
                                                            const int32_t *counts, const void *mma_a, const void *mma_b, void *mma_c,
                                                            int M, int F, int N2, int ldc, int B, int64_t cache_batch_stride,
                                                            void *stream) {
    CM_CHECK(packed && unpacked_colmajor && mma_a && mma_b && mma_c, "csp_mlp_mm2_and_scatter_add: null tensor pointer");
    if (int e = check_mlp_ragged(M, F, indices, counts)) return e;
    if (int e = check_mlp_batch(B, M)) return e;
    if (int e = check_cache_pitch(M, F, ldc)) return e;
    if (int e = check_cache_batch_stride(F, ldc, cache_batch_stride)) return e;
    CM_CHECK(N2 > 0 && N2 % 8 == 0, "mm2: N2 must be a positive multiple of 8 (got %d)", N2);   // before the first kernel is enqueued
    CM_CHECK((int64_t)M * F < (1ll << 31) && (int64_t)F * N2 < (1ll << 31), "mm2: M*F or F*N2 too large for 32-bit offsets");
    if (int e = launch_scatter_add_batched(packed, unpacked_colmajor, indices, counts, B, M, F, ldc, cache_batch_stride, (hipStream_t)stream))
        return e;
    return launch_mm2(mma_a, mma_b, mma_c, indices, counts, M, F, N2, (hipStream_t)stream, B);
}

// ---- GEMM2 over e4m3 rows of fc2^T (include/chipmunk_hip.h, "fp8 fc2")
extern "C" int chipmunk_csp_mlp_mm2_w8(const void *mma_a, const void *mma_b, const float *scale_b, void *mma_c, const int32_t *indices,
                                       const int32_t *counts, int M, int F, int N2, void *stream) {
    return launch_mm2_w8(mma_a, mma_b, scale_b, mma_c, indices, counts, M, F, N2, (hipStream_t)stream);
}
extern "C" int chipmunk_csp_mlp_mm2_w8_batched(const void *mma_a, const void *mma_b, const float *scale_b, void *mma_c,
                                               const int32_t *indices, const int32_t *counts, int M, int F, int N2, int B, void *stream) {
    CM_CHECK(B >= 1, "mlp: the batch size B must be at least 1 (got %d)", B);
    return launch_mm2_w8(mma_a, mma_b, scale_b, mma_c, indices, counts, M, F, N2, (hipStream_t)stream, B);
}

// ---- group-major activation cache (include/chipmunk_hip.h, "Group-major cache"): the *_gm entries.  The cache of sequence b is the
// [G, F, 128] block at pa_cache + b * cache_batch_stride; everything else is the *_batched entry's contract, B = 1 the single-sequence launch.
extern "C" int chipmunk_csp_mlp_mm1_act_gm(const void *a, const void *b, void *c, const void *bias, void *pa_cache, const int32_t *indices,
                                           const int32_t *counts, int M, int K, int F, int act, int update_cache, int B,
                                           int64_t cache_batch_stride, void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_act_entry(a, b, c, bias, pa_cache, indices, counts, nullptr, nullptr, false, M, K, F, BM, act, update_cache, (hipStream_t)stream,
                         B, cache_batch_stride, false, true);
}
extern "C" int chipmunk_csp_mlp_mm1_fp8_act_gm(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                               const int32_t *indices, const int32_t *counts, const float *scale_a, const float *scale_b,
                                               int M, int K, int F, int act, int update_cache, int B, int64_t cache_batch_stride,
                                               void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_act_entry(a, b, c, bias, pa_cache, indices, counts, scale_a, scale_b, true, M, K, F, BM, act, update_cache, (hipStream_t)stream,
                         B, cache_batch_stride, false, true);
}
extern "C" int chipmunk_csp_mlp_mm1_fp8_act_rs_gm(const void *a, const void *b, void *c, const void *bias, void *pa_cache,
                                                  const int32_t *indices, const int32_t *counts, const float *scale_a, const float *scale_b,
                                                  int M, int K, int F, int act, int update_cache, int B, int64_t cache_batch_stride,
                                                  void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_act_entry(a, b, c, bias, pa_cache, indices, counts, scale_a, scale_b, true, M, K, F, BM, act, update_cache, (hipStream_t)stream,
                         B, cache_batch_stride, true, true);
}
extern "C" int chipmunk_csp_mlp_mm1_glu_gm(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                                           const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts, int M, int K,
                                           int F, int act, int update_cache, int B, int64_t cache_batch_stride, void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_glu_entry(a, b_gate, b_up, c, bias_gate, bias_up, pa_cache, indices, counts, M, K, F, BM, act, update_cache,
                         (hipStream_t)stream, B, cache_batch_stride, true);
}
extern "C" int chipmunk_csp_mlp_mm1_glu_fp8_gm(const void *a, const void *b_gate, const void *b_up, void *c, const void *bias_gate,
                                               const void *bias_up, void *pa_cache, const int32_t *indices, const int32_t *counts,
                                               const float *scale_a, const float *scale_b_gate, const float *scale_b_up, int M, int K,
                                               int F, int act, int update_cache, int B, int64_t cache_batch_stride, void *stream) {
    if (int e = check_mlp_batch(B, M)) return e;
    return mm1_glu_fp8_entry(a, b_gate, b_up, c, bias_gate, bias_up, pa_cache, indices, counts, scale_a, scale_b_gate, scale_b_up, M, K, F, BM,
                             act, update_cache, (hipStream_t)stream, B, cache_batch_stride, true);
}
extern "C" int chipmunk_csp_scatter_add_gm(const void *packed, void *unpacked_groups, const int32_t *indices, const int32_t *counts, int M,
                                           int F, int B, int64_t cache_batch_stride, void *stream) {
    CM_CHECK(packed && unpacked_groups, "csp_scatter_add_gm: null tensor pointer");
    if (int e = check_mlp_ragged(M, F, indices, counts)) return e;
    if (int e = check_mlp_batch(B, M)) return e;
    if (int e = check_cache_groups(M, F, cache_batch_stride)) return e;
    if (B == 1) return launch_scatter_add(packed, unpacked_groups, indices, counts, M, F, BM, (hipStream_t)stream, F * BM);
    return launch_scatter_add_batched(packed, unpacked_groups, indices, counts, B, M, F, BM, cache_batch_stride, (hipStream_t)stream, F * BM);
}
extern "C" int chipmunk_transpose16_groups(const void *src, void *dst, int B, int R, int C, void *stream) {
    CM_CHECK(src && dst, "transpose16_groups: null tensor pointer");
    CM_CHECK(B > 0 && R > 0 && C > 0, "transpose16_groups: B, R and C must be positive (got %d, %d, %d)", B, R, C);
    CM_CHECK(B <= 65535 && (R + 127) / 128 <= 32767, "transpose16_groups: B must not exceed 65535 and ceil(R / 128) not 32767 (got B = %d, R = %d)",
             B, R);
    CM_CHECK((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "transpose16_groups: src and dst must be 16-byte aligned");
    hipLaunchKernelGGL(transpose16_groups_kernel, dim3((C + 63) / 64, 2 * ((R + 127) / 128), B), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t *)src, (uint16_t *)dst, R, C);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}
