// Indexed IO for gfx950: mask -> indices, top-k indices, indexed copy, bit packing.
// Replaces reference csrc/indexed_io/{mask_to_indices,topk_indices,copy_indices}.cu and ops/bitpack.py.
// HBM-bound integer/byte kernels: wide coalesced loads, wave64 ballots / popcounts instead of CUB scans,
// LDS for the per-row bit matrices.  Results are bit-exact against the reference's ordering rules.
#include "common.h"
#include "attn_params.h"

namespace {

// =====================================================================================  mask_to_indices
// Reference order (mask_to_indices.cu:49-86, one 32-lane warp per row): for residue class t = 0..31 all True columns
// c == t (mod 32) ascending, then padding with the first False columns ascending.
//
// Here one 256-thread workgroup per row:
//   A. each lane turns 32 mask bytes (one "i-row": columns 32i..32i+31) into a 32-bit word (bits[i] in LDS);
//   B. 32 wave64 ballots per 64 i-rows transpose the bit matrix: T[t][blk] = 64-bit vector of class t;
//   C. popcounts + a per-class scan over blocks + a scan over classes give every (class, block) cell its output offset;
//   D. each lane walks the set bits of its cell and writes the column numbers;
//   E. one lane appends the padding columns from the untransposed words.
// inclusive prefix sum over the 64 lanes in six DPP adds (row_shr 1/2/4/8 inside the 16-lane rows, row_bcast:15 and :31
// across them) -- the __shfl_up form is six ds_bpermute round trips through the LDS crossbar, each with its index
// arithmetic and select, and the sorted compaction below runs two such chains per 2 048 columns.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);
    return x;
}
struct M2IParams {
    const uint8_t *mask;  // bool bytes [rows, n]  (PACKED == false)  or packed bits [rows*n/8] (PACKED == true)
    int32_t *indices;
    int32_t *counts;
    int n, pad_n, multiple_of;
    const int64_t *offsets;  // RAGGED: row r goes to indices + offsets[r], offsets[r + 1] - offsets[r] entries wide
};

// SORTED = true emits the kept columns in ASCENDING order instead (same set, same counts, same padding columns): not
// the reference's order, but the attention result does not depend on it and ascending keys turn the K/V gather into
// near-sequential DRAM pages (measured 1.6x on the C3 sparse step).  Used by SparseDiffAttn's fused path only.
// RAGGED = true writes the row into ragged rows (the layout of compact_indices_kernel below) instead of a row of the padded
// [rows, pad_n] tensor: same entries in the same order, then ZEROS from the last valid entry (kept + padding columns, at most
// n) to the end of the row; counts are mask_row_counts_kernel's and are not written again.  Nothing is written past the row's
// width, whatever the offsets say, and a row of width 0 is not even read.
template <bool PACKED, bool SORTED = false, bool RAGGED = false>
__global__ __launch_bounds__(256) void mask_to_indices_kernel(const M2IParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = p.n;
    const int NI = (n + 31) >> 5;   // 32-column words per row
    const int NB = (NI + 63) >> 6;  // 64-word blocks per row
    uint32_t *bits = (uint32_t *)smem;                               // [NB*64]
    unsigned long long *T = (unsigned long long *)(bits + NB * 64);  // [32][NB]
    uint32_t *pre = (uint32_t *)(T + 32 * NB);                       // [32][NB] exclusive offsets
    uint32_t *cls = pre + 32 * NB;                                   // [33] class totals / offsets

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t row = blockIdx.x;
    int32_t *out = p.indices + row * p.pad_n;
    int width = 0;
    if constexpr (RAGGED) {
        const int64_t o = p.offsets[row];
        out = p.indices + o;
        width = (int)min((int64_t)0x7fffffff, p.offsets[row + 1] - o);
        if (width <= 0) return;
    }
    auto put = [&](int pos, int col) {
        if (!RAGGED || pos < width) out[pos] = col;
    };
    // RAGGED: zeros behind the `total` kept columns and the padding columns (which run out at n)
    auto zero_rest = [&](int total) {
        const int rem = total % p.multiple_of;
        const int64_t padded = rem ? (int64_t)total - rem + p.multiple_of : total;
        for (int i = (int)min(padded, (int64_t)n) + tid; i < width; i += 256) out[i] = 0;
    };

    // ---- A: bit words
    if constexpr (PACKED) {
        const uint8_t *src = p.mask + ((row * n) >> 3);  // n % 8 == 0 guaranteed by the host
        const bool aligned4 = ((((uintptr_t)src) & 3) == 0);
        for (int i = tid; i < NB * 64; i += 256) {
            uint32_t word = 0;
            if (i < NI) {
                const int nbytes = min(4, (n - i * 32 + 7) >> 3);
                if (aligned4 && nbytes == 4) {
                    word = *(const uint32_t *)(src + i * 4);
                } else {
                    for (int j = 0; j < nbytes; ++j) word |= (uint32_t)src[i * 4 + j] << (8 * j);
                }
                const int rem = n - i * 32;
                if (rem < 32) word &= (1u << rem) - 1u;
            }
            bits[i] = word;
        }
    } else {
        const uint8_t *src = p.mask + row * n;
        const bool aligned16 = ((((uintptr_t)src) & 15) == 0);
        for (int i = tid; i < NB * 64; i += 256) {
            uint32_t word = 0;
            if (i < NI) {
                if (aligned16 && i * 32 + 32 <= n) {
                    const u32x4 lo = *(const u32x4 *)(src + i * 32);
                    const u32x4 hi = *(const u32x4 *)(src + i * 32 + 16);
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        // bool bytes are 0/1 (any non-zero counts as true): gather bit 0 of the 4 bytes of each dword
                        uint32_t x = lo[d], y = hi[d];
                        x = (x | (x >> 1) | (x >> 2) | (x >> 3) | (x >> 4) | (x >> 5) | (x >> 6) | (x >> 7)) & 0x01010101u;
                        y = (y | (y >> 1) | (y >> 2) | (y >> 3) | (y >> 4) | (y >> 5) | (y >> 6) | (y >> 7)) & 0x01010101u;
                        const uint32_t nx = (x | (x >> 7) | (x >> 14) | (x >> 21)) & 0xfu;
                        const uint32_t ny = (y | (y >> 7) | (y >> 14) | (y >> 21)) & 0xfu;
                        word |= nx << (4 * d);
                        word |= ny << (16 + 4 * d);
                    }
                } else {
                    const int rem = min(32, n - i * 32);
                    for (int j = 0; j < rem; ++j) word |= (uint32_t)(src[i * 32 + j] != 0) << j;
                }
            }
            bits[i] = word;
        }
    }
    __syncthreads();

    if constexpr (SORTED) {
        // ordered compaction, wave-cooperative: a wave takes 64 consecutive words (2048 columns) at a time, lane = word.
        // Pass 1: popcount per word -> per-block totals in LDS; one wave scans the (<= 64 per step) block totals.
        // Pass 2: wave prefix of the lane popcounts + block base = every word's output offset; lanes walk their set bits.
        // Consecutive lanes write consecutive output runs, so a wave's store instruction covers a few cache lines (the
        // per-thread-chunk form wrote 256 separate streams per row: 0.95 ms per C3 layer).
        uint32_t *blktot = (uint32_t *)T;   // [NB + 1] (the transpose matrix is not used by this variant)
        for (int blk = w; blk < NB; blk += 4) {
            const uint32_t c = wave_incl_scan(__popc(bits[blk * 64 + lane]));
            if (lane == 63) blktot[blk] = c;
        }
        __syncthreads();
        if (w == 0) {   // exclusive scan of the block totals, 64 blocks per step
            uint32_t run = 0;
            for (int b0 = 0; b0 < NB; b0 += 64) {
                const uint32_t v = b0 + lane < NB ? blktot[b0 + lane] : 0u;
                const uint32_t incl = wave_incl_scan(v);
                if (b0 + lane < NB) blktot[b0 + lane] = run + incl - v;
                run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
            if (lane == 0) blktot[NB] = run;
        }
        __syncthreads();
        const int total = (int)blktot[NB];
        for (int blk = w; blk < NB; blk += 4) {
            uint32_t v = bits[blk * 64 + lane];
            const uint32_t c = __popc(v);
            const uint32_t incl = wave_incl_scan(c);
            int pos = (int)(blktot[blk] + incl - c);
            const int col0 = (blk * 64 + lane) * 32;
            while (v) {
                const int bit = __builtin_ctz(v);
                v &= v - 1;
                put(pos++, col0 + bit);
            }
        }
        if constexpr (RAGGED) zero_rest(total);
        if (tid == 0) {
            const int padded = ((total + p.multiple_of - 1) / p.multiple_of) * p.multiple_of;
            int pp = total;
            for (int i = 0; i < NI && pp < padded; ++i) {
                uint32_t z = ~bits[i];
                const int rem = n - i * 32;
                if (rem < 32) z &= (1u << rem) - 1u;
                while (z && pp < padded) {
                    const int bit = __builtin_ctz(z);
                    z &= z - 1;
                    put(pp++, i * 32 + bit);
                }
            }
            if constexpr (!RAGGED) p.counts[row] = padded;
        }
        return;
    }
    // ---- B: transpose by ballots (each wave takes blocks w, w+4, ...)
    for (int blk = w; blk < NB; blk += 4) {
        const uint32_t word = bits[blk * 64 + lane];
        unsigned long long mine = 0;
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const unsigned long long bal = __ballot((word >> t) & 1u);
            if (lane == t) mine = bal;
        }
        if (lane < 32) T[lane * NB + blk] = mine;
    }
    __syncthreads();

    // ---- C: offsets.  One lane per class scans its blocks; then 32 classes are scanned by lane 0.
    if (tid < 32) {
        uint32_t run = 0;
        for (int blk = 0; blk < NB; ++blk) {
            pre[tid * NB + blk] = run;
            run += __popcll(T[tid * NB + blk]);
        }
        cls[tid + 1] = run;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int t = 0; t < 32; ++t) {
            const uint32_t c = cls[t + 1];
            cls[t] = run;  // exclusive class offset (cls[t+1] is consumed before it is overwritten next iteration)
            run += c;
            if (t == 31) cls[32] = run;
        }
    }
    __syncthreads();
    const int total = (int)cls[32];

    // ---- D: emit.  Consecutive lanes take consecutive blocks of one class => neighbouring output runs.
    for (int cell = tid; cell < 32 * NB; cell += 256) {
        const int t = cell / NB, blk = cell - t * NB;
        unsigned long long v = T[cell];
        int pos = (int)(cls[t] + pre[cell]);
        while (v) {
            const int bit = __builtin_ctzll(v);
            v &= v - 1;
            put(pos++, ((blk * 64 + bit) << 5) + t);
        }
    }
    if constexpr (RAGGED) zero_rest(total);

    // ---- E: padding with the first False columns (lane 0 only, <= multiple_of-1 columns)
    if (tid == 0) {
        const int padded = ((total + p.multiple_of - 1) / p.multiple_of) * p.multiple_of;
        int pos = total;
        for (int i = 0; i < NI && pos < padded; ++i) {
            uint32_t z = ~bits[i];
            const int rem = n - i * 32;
            if (rem < 32) z &= (1u << rem) - 1u;
            while (z && pos < padded) {
                const int bit = __builtin_ctz(z);
                z &= z - 1;
                put(pos++, i * 32 + bit);
            }
        }
        if constexpr (!RAGGED) p.counts[row] = padded;
    }
}

// kept columns per row, rounded as mask_to_indices_kernel rounds them, and the width the row takes in ragged rows -- what the caller
// needs to lay the rows out before anything is emitted.  One wave per row, four rows per workgroup: 16 bytes per lane and step (head
// and tail bytes one per lane: packed rows of n % 32 != 0 columns start at any byte), popcounts, one DPP reduction.
struct RowCountParams {
    const uint8_t *mask;  // as M2IParams
    int32_t *counts;      // [rows] kept columns rounded up to multiple_of (may exceed n)
    int64_t *lengths;     // [rows] min(counts, pad_n) rounded up to 32
    int64_t rows;
    int n, pad_n, multiple_of;
};

template <bool PACKED>
__global__ __launch_bounds__(256) void mask_row_counts_kernel(const RowCountParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;   // the whole wave
    const int nbytes = PACKED ? p.n >> 3 : p.n;
    const uint8_t *src = p.mask + (PACKED ? (row * p.n) >> 3 : row * p.n);
    auto set_in_byte = [](uint32_t b) { return PACKED ? (uint32_t)__popc(b) : (uint32_t)(b != 0); };
    auto set_in_word = [](uint32_t x) {
        if constexpr (!PACKED) x = (x | (x >> 1) | (x >> 2) | (x >> 3) | (x >> 4) | (x >> 5) | (x >> 6) | (x >> 7)) & 0x01010101u;
        return (uint32_t)__popc(x);
    };
    const int head = min(nbytes, (int)((16 - ((uintptr_t)src & 15)) & 15));
    uint32_t cnt = lane < head ? set_in_byte(src[lane]) : 0u;
    const int nvec = (nbytes - head) >> 4;
    const u32x4 *vec = (const u32x4 *)(src + head);
#pragma unroll 4
    for (int i = lane; i < nvec; i += 64) {
        const u32x4 x = vec[i];
        cnt += set_in_word(x[0]) + set_in_word(x[1]) + set_in_word(x[2]) + set_in_word(x[3]);
    }
    const int tail = head + (nvec << 4) + lane;   // fewer than 16 bytes are left
    if (tail < nbytes) cnt += set_in_byte(src[tail]);
    const int64_t kept = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(cnt), 63);
    if (lane == 0) {
        const int64_t padded = ((kept + p.multiple_of - 1) / p.multiple_of) * p.multiple_of;
        p.counts[row] = (int32_t)padded;
        p.lengths[row] = (min(padded, (int64_t)p.pad_n) + 31) / 32 * 32;
    }
}

// =====================================================================================  topk_indices
struct TopkParams {
    const void *act;
    void *cache;  // DELTA variant: the block-mean cache the activations are compared with and copied into
    int32_t *indices;
    int32_t *counts;
    int rows, cols, multiple_of;
    float quantile, random_amount;
    uint32_t salt;  // per-launch value (host counter mixed with the seed, see chipmunk_next_random_salt)
    // GROUP form only: act / cache are [batches, src_rows, cols]; workgroup b * groups + g owns rows [g * group_rows, (g + 1) * group_rows)
    // of sequence b, cut at src_rows (the last group may be short)
    int group_rows, src_rows, groups;
};

template <typename T>
__device__ __forceinline__ float load_as_float(const T *p, int i);
template <>
__device__ __forceinline__ float load_as_float<uint16_t>(const uint16_t *p, int i) { return bf16_bits_to_f32(p[i]); }
template <>
__device__ __forceinline__ float load_as_float<_Float16>(const _Float16 *p, int i) { return (float)p[i]; }
template <>
__device__ __forceinline__ float load_as_float<float>(const float *p, int i) { return p[i]; }

template <typename T>
__device__ __forceinline__ float round_to(float x);
template <>
__device__ __forceinline__ float round_to<uint16_t>(float x) { return round_bf16(x); }
template <>
__device__ __forceinline__ float round_to<_Float16>(float x) { return (float)(_Float16)x; }
template <>
__device__ __forceinline__ float round_to<float>(float x) { return x; }

// counter-based uniform in [0,1): replaces cuRAND Philox of topk_indices.cu:46-49,108 (RNG streams cannot match).
// `salt` changes with every launch (host counter + seed) and with the row's data (its first element, as the reference
// seeds cuRAND from the first activation word, topk_indices.cu:47-49): the random keys exist to refresh stale cache
// columns over time, so the chosen set must differ between layers, steps and generations.
__device__ __forceinline__ float hash_uniform(uint32_t row, uint32_t col, uint32_t salt) {
    uint32_t x = (row * 0x9E3779B9u ^ (col + 0x7F4A7C15u) * 0x85EBCA6Bu) + salt * 0xC2B2AE35u;
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return (float)(x >> 8) * (1.0f / 16777216.0f);
}

// Block-wide ordered compaction step for a 1024-thread workgroup (16 waves): returns this thread's output slot (or
// -1) and advances `base`.  One ballot + popcount per wave, the 16 wave totals are scanned through LDS.
__device__ __forceinline__ int compact_slot(bool keep, int lane, int w, uint32_t *wave_tot, int &base) {
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[w] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = wave_tot[i];
        off += i < w ? c : 0;
        tot += c;
    }
    __syncthreads();
    base += tot;
    return keep ? off + before : -1;
}

// One 1024-thread workgroup per row (the reference's launch shape, topk_indices.cu:200-213).  The quantile of the
// 1024-column sample is found by rank counting (each thread ranks its own sample against all 1024 through LDS
// broadcasts) instead of the reference's CUB block merge sort: same element, ~1 us.
// DELTA = true fuses the sparse-MLP sequence |bmfc1 - cache| -> topk_indices -> copy_indices (reference
// modules/mlp.py:70-85 with bm == mbm): the ranked value is |T(b - cache)| computed on the fly and every selected
// column (padding included, like copy_indices) is copied into the cache by the thread that owns it.
//
// TOPP = true is the `_p` form (mlp.top_p; not in the reference): a column count per row from the row's mass.  With m_c = v_c where
// v_c > 0 (a zero, negative or NaN entry carries none), total = sum of m_c over the WHOLE row and target = float(top_p) * total,
//   thr_p   = the largest t with sum{m_c : v_c >= t} >= target (a class of equal values is taken whole); +inf when total == 0
//   thr_q   = the threshold above (k_q = int(1024 * sparsity)); -inf for sparsity == 0: no cap
//   thr_min = the same order statistic at k_min = int(1024 * (1 - min_keys)) (the host keeps k_min >= k_q); +inf for k_min >= 1024
//   kept    : m_c > 0 and v_c >= min(max(thr_p, thr_q), thr_min)
// and the random keys, the padding and the order follow as in the plain form.  Same launch shape and first-pass loads: the 16 values a
// thread already holds become its masses; the row total and every bisection round are one block-wide fp32 sum in a FIXED order (a
// thread's columns ascending, the wave by row16_sum / sum_across_rows, the 16 wave partials ascending through LDS) -- no floating-point
// atomics, the same launch gives the same bits, and a fixed-order sum of non-negative terms is monotone in the set summed, so the
// bisection over the order-preserving key bits is well defined.  thr_p is the key of a column, and every key of a positive bf16 / fp16
// value has its low 16 / 13 bits zero (the plain form too: only positive values carry mass), so the rounds stop above them: 15 rounds
// for bf16, 18 for fp16, 31 for fp32.  Columns past 16 384 do not fit the registers: every round reads them again (L2 hits; FLUX,
// HunyuanVideo and Wan rows are 12 288 - 13 824 columns and have none).  Lanes past the row's end hold zeros: no mass, no load.
struct TopkPParams : TopkParams {
    float top_p;
    int k_min;  // index of thr_min in the sorted sample; >= 1024: no floor
};

// GROUP = true (with DELTA; topk_group_delta_indices, not in the reference) is the delta form over the nr <= group_rows block-mean rows
// a 128-row group owns (bm > mbm, and the gate / up pairs of the gated MLP): the ranked value of column c is
//     s_c = T( sum_i float( T(|b_i[c] - cache_i[c]|) ) ),   i ascending over the group's rows, fp32, rounded to T once
// -- what (b - cache).abs().reshape(B, G, R, F).sum(2) gives for R = 2 bit for bit (one fp32 add, one rounding), and for R = 1 the
// plain delta form's value.  The sum starts at +0: the terms are |.|, never -0, so 0 + t_0 is t_0 in every bit (NaN included).  The
// scores are non-negative and rounded to T, so the low-bit shortcuts below hold; the workgroup (one per (sequence, group)) lists into
// row b * groups + g of indices / counts and copies a listed column in every row the group owns.  The first pass walks the rows in the
// outer loop, so a thread has its 16 columns of a row in flight at once; columns past 16 384 are summed again where they are needed.
template <typename T, bool DELTA, bool TOPP = false, bool GROUP = false>
__global__ __launch_bounds__(1024) void topk_indices_kernel(const typename std::conditional<TOPP, TopkPParams, TopkParams>::type p) {
    static_assert(DELTA || !GROUP, "the group form is a delta form");
    __shared__ uint32_t wave_tot[16];
    __shared__ float thr_s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = blockIdx.x;
    const int cols = p.cols;
    int64_t first = row;   // first row of act / cache this workgroup reads
    int nr = 1;            // ... and how many
    if constexpr (GROUP) {
        const int b = row / p.groups, g = row - b * p.groups;
        first = (int64_t)b * p.src_rows + (int64_t)g * p.group_rows;
        nr = min(p.group_rows, p.src_rows - g * p.group_rows);
    }
    const T *x = (const T *)p.act + first * cols;
    T *xc = DELTA ? (T *)p.cache + first * cols : nullptr;
    int32_t *out = p.indices + (int64_t)row * cols;
    auto value = [&](int c) {
        if constexpr (GROUP) {
            float s = 0.f;
            for (int i = 0; i < nr; ++i)
                s += fabsf(round_to<T>(load_as_float<T>(x + (int64_t)i * cols, c) - load_as_float<T>(xc + (int64_t)i * cols, c)));
            return round_to<T>(s);
        } else {
            const float b = load_as_float<T>(x, c);
            if constexpr (DELTA) return fabsf(round_to<T>(b - load_as_float<T>(xc, c)));
            else return b;
        }
    };
    auto refresh = [&](int c) {  // DELTA: column c of the activations into the cache, in every row this workgroup owns
        if constexpr (GROUP) {
            for (int i = 0; i < nr; ++i) xc[(int64_t)i * cols + c] = x[(int64_t)i * cols + c];
        } else {
            xc[c] = x[c];
        }
    };

    const uint32_t salt = p.salt ^ (__float_as_uint(value(0)) * 0x27D4EB2Fu);  // the fused (delta) form sees what the unfused op sees
    if (!TOPP && p.quantile == 0.f) {  // keep everything (topk_indices.cu:51-59); the _p form has no cap there and still selects by mass
        if constexpr (DELTA)
            for (int c = tid; c < cols; c += 1024) refresh(c);
        for (int c = tid; c < cols; c += 1024) out[c] = c;
        if (tid == 0) p.counts[row] = cols;
        return;
    }
    if (p.quantile == 1.f) {  // keep nothing (topk_indices.cu:60-69)
        for (int c = tid; c < cols; c += 1024) out[c] = -1;
        if (tid == 0) p.counts[row] = 0;
        return;
    }
    // ---- threshold = element int(1024*q) of the ascending-sorted first 1024 values (topk_indices.cu:91-101).
    //      Order statistic by bitwise bisection inside ONE wave (16 sample keys per lane, no barriers, no sort):
    //      result = largest v with #{keys < v} <= k, built from the most significant bit down.
    // every thread first requests the 16 columns it will test in the first compaction pass (t, t + 1024, ...): column
    // t of that batch is also its share of the 1024-column quantile sample, handed to wave 0 through LDS -- one memory
    // round trip for sample and first pass instead of two (the rows are cold in the real loop: 31 -> 25 us)
    __shared__ float sample[1024];
    float v_first[16];
    if constexpr (GROUP) {
#pragma unroll
        for (int j = 0; j < 16; ++j) v_first[j] = 0.f;
        for (int i = 0; i < nr; ++i) {
            const T *xi = x + (int64_t)i * cols, *ci = xc + (int64_t)i * cols;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = j * 1024 + tid;
                if (c < cols) v_first[j] += fabsf(round_to<T>(load_as_float<T>(xi, c) - load_as_float<T>(ci, c)));
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) v_first[j] = round_to<T>(v_first[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = j * 1024 + tid;
            v_first[j] = c < cols ? value(c) : 0.f;
        }
    }
    sample[tid] = v_first[0];
    if constexpr (TOPP) {
        // ---- masses in place of the values (the sample keeps the values as they are), row total, thr_q / thr_min, thr_p
        __shared__ float part[2][16];
        __shared__ float thr_qm[2];
        auto block_sum = [&](float s, int buf) {  // every thread gets the same bits; one barrier (the buffers alternate)
            s = sum_across_rows(row16_sum(s));
            if (lane == 0) part[buf][w] = s;
            __syncthreads();
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) t += part[buf][i];
            return t;
        };
        // mass of the columns >= key `cand` (cand >= 1; a column without mass has key 0)
        auto mass_from = [&](uint32_t cand) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) s += __float_as_uint(v_first[j]) >= cand ? v_first[j] : 0.f;
            for (int c = 16 * 1024 + tid; c < cols; c += 1024) {
                const float v = value(c);
                s += (v > 0.f && __float_as_uint(v) >= cand) ? v : 0.f;
            }
            return s;
        };
#pragma unroll
        for (int j = 0; j < 16; ++j) v_first[j] = v_first[j] > 0.f ? v_first[j] : 0.f;
        const float total = block_sum(mass_from(1u), 0);  // (the barrier inside also publishes the sample)
        if (w == 0) {
            uint32_t key[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t u = __float_as_uint(sample[lane + 64 * j]);
                key[j] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // monotone float -> unsigned map
            }
            // both order statistics in one loop: the two counts (<= 1024 each) ride one wave sum as cnt_q + 2048 * cnt_min, exact in fp32
            const int kq = (int)(1024 * p.quantile), km = p.k_min;
            uint32_t rq = 0, rm = 0;
            // (the one round for the LOWZ low bits of a 16-bit |delta|: see the plain form below)
            constexpr int LOWZ = !DELTA ? 0 : std::is_same<T, uint16_t>::value ? 16 : std::is_same<T, _Float16>::value ? 13 : 0;
            constexpr int LAST = LOWZ ? LOWZ - 1 : 0;
            for (int bit = 31; bit >= LAST; --bit) {
                const uint32_t add = LOWZ && bit == LAST ? (1u << LOWZ) - 1u : (1u << bit);
                const uint32_t cq = rq | add, cm = rm | add;
                int cnt = 0;
#pragma unroll
                for (int j = 0; j < 16; ++j) cnt += (key[j] < cq ? 1 : 0) + (key[j] < cm ? 2048 : 0);
                const int tot = (int)sum_across_rows(row16_sum((float)cnt));
                if ((tot & 2047) <= kq) rq = cq;
                if ((tot >> 11) <= km) rm = cm;
            }
            if (lane == 0) {
                const uint32_t uq = (rq & 0x80000000u) ? (rq & 0x7fffffffu) : ~rq, um = (rm & 0x80000000u) ? (rm & 0x7fffffffu) : ~rm;
                thr_qm[0] = p.quantile == 0.f ? -INFINITY : __uint_as_float(uq);
                thr_qm[1] = km >= 1024 ? INFINITY : __uint_as_float(um);
            }
        }
        // thr_p: the largest key whose columns carry the target, from the exponent's top bit down (bit 31 of every positive key's
        // image is set, the sign bit of the float itself clear: the search runs over the float's own bits)
        constexpr int LOWZ_P = std::is_same<T, uint16_t>::value ? 16 : std::is_same<T, _Float16>::value ? 13 : 0;
        const float target = p.top_p * total;
        uint32_t res = 0;
        for (int bit = 30; bit >= LOWZ_P; --bit) {
            const uint32_t cand = res | (1u << bit);
            if (block_sum(mass_from(cand), (bit & 1) ^ 1) >= target) res = cand;
        }
        const float thr_p = total > 0.f ? __uint_as_float(res) : INFINITY;
        if (tid == 0) thr_s = fminf(fmaxf(thr_p, thr_qm[0]), thr_qm[1]);  // (thr_qm: this thread's own stores)
    } else {
        __syncthreads();
    }
    if (!TOPP && w == 0) {
        uint32_t key[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t u = __float_as_uint(sample[lane + 64 * j]);
            key[j] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // monotone float -> unsigned map
        }
        const int k = (int)(1024 * p.quantile);
        uint32_t res = 0;
        // |delta| rounded to a 16-bit type: every key is a non-negative float whose LOWZ low bits are zero (bf16: 16, fp16: 13), so
        // the LOWZ low rounds all ask the same question (#{key <= res} <= k ?) and set all of their bits or none -- one round
        // decides them, same result bit for bit, 17 rounds instead of 32
        constexpr int LOWZ = !DELTA ? 0 : std::is_same<T, uint16_t>::value ? 16 : std::is_same<T, _Float16>::value ? 13 : 0;
        constexpr int LAST = LOWZ ? LOWZ - 1 : 0;
        for (int bit = 31; bit >= LAST; --bit) {
            const uint32_t cand = res | (LOWZ && bit == LAST ? (1u << LOWZ) - 1u : (1u << bit));
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) cnt += key[j] < cand ? 1 : 0;
            // wave total by DPP row rotations + two lane swaps (exact in fp32: <= 1024).  Six __shfl_xor steps are six ds_bpermute round
            // trips per round, 32 rounds in a row on one wave while the other 15 wait: ~10 us of this kernel's 19 (round 4)
            const int tot = (int)sum_across_rows(row16_sum((float)cnt));
            if (tot <= k) res = cand;
        }
        const uint32_t u = (res & 0x80000000u) ? (res & 0x7fffffffu) : ~res;
        if (lane == 0) thr_s = __uint_as_float(u);
    }
    __syncthreads();
    const float thr = thr_s;

    // ---- ordered compaction of kept columns, 16 x 1024 columns per pass: every thread tests up to 16 columns
    //      (t, t+1024, ...: all loads in flight at once), one ballot per (chunk, wave), ONE scan of the 256 wave totals.
    __shared__ uint32_t tot[16 * 16 + 1];
    int base = 0;
    int my_last_invalid = -1;
    for (int pass0 = 0; pass0 < cols; pass0 += 16 * 1024) {
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = pass0 + j * 1024 + tid;
            v[j] = pass0 == 0 ? v_first[j] : (c < cols ? value(c) : 0.f);
        }
        uint32_t keepbits = 0;
        int before[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = pass0 + j * 1024 + tid;
            bool keep = false;
            if (c < cols) {
                keep = TOPP ? (v[j] > 0.f && v[j] >= thr) : v[j] >= thr;
                if (!keep && p.random_amount > 0.f) keep = hash_uniform(row, c, salt) < p.random_amount;
                if (!keep) my_last_invalid = c;  // ascending c per thread => ends as the last rejected column
            }
            const unsigned long long bal = __ballot(keep);
            before[j] = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) tot[j * 16 + w] = __popcll(bal);
            keepbits |= keep ? (1u << j) : 0u;
        }
        __syncthreads();
        if (tid < 64) {  // exclusive scan of the 256 (chunk, wave) totals by one wave, 4 entries per lane
            uint32_t a0 = tot[tid * 4], a1 = tot[tid * 4 + 1], a2 = tot[tid * 4 + 2], a3 = tot[tid * 4 + 3];
            uint32_t sum = a0 + a1 + a2 + a3, incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if (lane >= d) incl += o;
            }
            const uint32_t excl = incl - sum;
            tot[tid * 4] = excl, tot[tid * 4 + 1] = excl + a0, tot[tid * 4 + 2] = excl + a0 + a1;
            tot[tid * 4 + 3] = excl + a0 + a1 + a2;
            if (tid == 63) tot[256] = incl;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (keepbits & (1u << j)) {
                const int c = pass0 + j * 1024 + tid;
                out[base + tot[j * 16 + w] + before[j]] = c;
                if constexpr (DELTA) refresh(c);
            }
        base += tot[256];
        __syncthreads();
    }
    const int kept = base;
    const int mod = kept % p.multiple_of;
    const int pad = mod == 0 ? 0 : p.multiple_of - mod;
    if (tid == 0) p.counts[row] = kept + pad;
    // ---- padding candidates in ascending residue order (a deterministic choice among the reference's outcomes)
    if (pad > 0) {
        int pbase = 0;
        const int slot = compact_slot(my_last_invalid != -1, lane, w, wave_tot, pbase);
        if (slot >= 0 && slot < pad) {
            out[kept + slot] = my_last_invalid;
            if constexpr (DELTA) refresh(my_last_invalid);
        }
    }
}

// =====================================================================================  copy_indices
template <typename T>
__global__ __launch_bounds__(256) void copy_indices_kernel(const T *src, T *dst, const int32_t *inds,
                                                           const int32_t *counts, int M, int R, int F) {
    const int64_t grow = blockIdx.x;                 // row over B*M*R
    const int64_t b = grow / ((int64_t)M * R);
    const int base_m = (int)((grow % ((int64_t)M * R)) / R);
    const int cnt = counts[b * M + base_m];
    const int32_t *ii = inds + (b * M + base_m) * (int64_t)F;
    for (int c = threadIdx.x; c < cnt; c += 256) {
        const int col = ii[c];
        dst[grow * F + col] = src[grow * F + col];
    }
}

// =====================================================================================  bitpack / bitunpack
__global__ __launch_bounds__(256) void bitpack_kernel(const uint8_t *mask, uint8_t *packed, int64_t n) {
    const int64_t nb = (n + 7) >> 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (int64_t)gridDim.x * 256) {
        uint8_t byte = 0;
        if (i * 8 + 8 <= n && ((((uintptr_t)mask) & 7) == 0)) {
            unsigned long long v = *(const unsigned long long *)(mask + i * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) byte |= (uint8_t)((((v >> (8 * j)) & 0xffull) != 0) << j);
        } else {
            for (int j = 0; j < 8 && i * 8 + j < n; ++j) byte |= (uint8_t)((mask[i * 8 + j] != 0) << j);
        }
        packed[i] = byte;
    }
}
__global__ __launch_bounds__(256) void bitunpack_kernel(const uint8_t *packed, uint8_t *mask, int64_t n) {
    const int64_t nb = (n + 7) >> 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (int64_t)gridDim.x * 256) {
        const uint8_t byte = packed[i];
        if (i * 8 + 8 <= n && ((((uintptr_t)mask) & 7) == 0)) {
            unsigned long long v = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) v |= (unsigned long long)((byte >> j) & 1u) << (8 * j);
            *(unsigned long long *)(mask + i * 8) = v;
        } else {
            for (int j = 0; j < 8 && i * 8 + j < n; ++j) mask[i * 8 + j] = (byte >> j) & 1u;
        }
    }
}

// =====================================================================================  2-byte transpose
// [B, R, C] -> [B, C, R] for 16-bit elements (the column-major activation cache of the sparse MLP is act^T,
// reference modules/mlp.py:56).  64x64 tiles through LDS: 128-byte row segments on both the read and the write side.
// The output rows have a pitch of ld >= R elements; elements [R, ld) of every row are written as zeros (the tile rows past R are).
__global__ __launch_bounds__(256) void transpose16_kernel(const uint16_t *src, uint16_t *dst, int R, int C, int ld) {
    __shared__ __attribute__((aligned(16))) uint16_t tile[64][72];
    const int64_t boff = (int64_t)blockIdx.z * R * C;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int item = i * 256 + tid, r = item >> 3, ch = item & 7;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r0 + r < R && c0 + ch * 8 + 8 <= C) v = *(const u32x4 *)(src + boff + (int64_t)(r0 + r) * C + c0 + ch * 8);
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
        uint16_t *d = dst + (int64_t)blockIdx.z * C * ld + (int64_t)(c0 + c) * ld + r0 + ch * 8;
        if (r0 + ch * 8 + 8 <= ld && ((ld & 7) == 0)) *(u32x4 *)d = *(const u32x4 *)&tile[c][ch * 8];
        else
            for (int e = 0; e < 8; ++e)
                if (r0 + ch * 8 + e < ld) d[e] = tile[c][ch * 8 + e];
    }
}

// ragged copy of index rows: row r of `flat` (at offsets[r]) = the first counts[r] entries of row r of `indices`, the rest of
// the row (up to offsets[r + 1]) zero.  One workgroup per row, 16 bytes per lane when both sides allow.
__global__ __launch_bounds__(256) void compact_indices_kernel(const int32_t *indices, int64_t idx_stride, const int32_t *counts,
                                                             const int64_t *offsets, int32_t *flat) {
    const int64_t r = blockIdx.x;
    const int32_t *src = indices + r * idx_stride;
    const int64_t o = offsets[r];
    int32_t *dst = flat + o;
    const int width = (int)(offsets[r + 1] - o);
    int c = counts[r];
    c = c < 0 ? 0 : (c < width ? c : width);
    c = c < idx_stride ? c : (int)idx_stride;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const int c4 = c >> 2;
        for (int i = threadIdx.x; i < c4; i += 256) ((u32x4 *)dst)[i] = ((const u32x4 *)src)[i];
        for (int i = (c4 << 2) + threadIdx.x; i < c; i += 256) dst[i] = src[i];
    } else {
        for (int i = threadIdx.x; i < c; i += 256) dst[i] = src[i];
    }
    for (int i = c + threadIdx.x; i < width; i += 256) dst[i] = 0;
}

size_t m2i_lds_bytes(int n, bool sorted) {
    const int NI = (n + 31) >> 5, NB = (NI + 63) >> 6;
    if (sorted) return (size_t)NB * 64 * 4 + (size_t)(NB + 1) * 4 + 16;   // bit words + block totals: 8 workgroups per CU
    return (size_t)NB * 64 * 4 + (size_t)32 * NB * 8 + (size_t)32 * NB * 4 + 33 * 4 + 16;
}

template <bool PACKED, bool SORTED = false, bool RAGGED = false>
int launch_m2i(const void *mask, int32_t *indices, int32_t *counts, int64_t rows, int n, int pad_n, int multiple_of,
               void *stream, const int64_t *offsets = nullptr) {
    CM_CHECK(mask && indices && (RAGGED ? (const void *)offsets : (const void *)counts), "mask_to_indices: null pointer");
    CM_CHECK(rows >= 0 && n > 0 && pad_n >= n && multiple_of > 0, "mask_to_indices: bad sizes rows=%lld n=%d pad_n=%d multiple_of=%d",
             (long long)rows, n, pad_n, multiple_of);
    CM_CHECK(rows < (1ll << 31), "mask_to_indices: too many rows");
    if (PACKED) CM_CHECK(n % 8 == 0, "packed_mask_to_indices: n must be a multiple of 8 (got %d)", n);
    const size_t lds = m2i_lds_bytes(n, SORTED);
    CM_CHECK(lds <= 160 * 1024, "mask_to_indices: row length %d needs %zu B of LDS (> 160 KiB)", n, lds);
    if (rows == 0) return CHIPMUNK_OK;
    auto kern = mask_to_indices_kernel<PACKED, SORTED, RAGGED>;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    M2IParams p = {(const uint8_t *)mask, indices, counts, n, pad_n, multiple_of, offsets};
    hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(256), lds, (hipStream_t)stream, p);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}


// ------------------------------------------------------------------------------------------------ top-k -> mask
// SURVEY 8f rank 1, second half: the reference's `random_and_topk` (src/chipmunk/modules/attn.py:76-82)
//     mask = randint(0,100) == 0;  mask.scatter_(-1, cs.topk(k).indices, True);  mask = (mask * groups) | static
// as ONE pass over the column sums instead of randint + topk + scatter + two element-wise kernels on a [H, G, N] bool
// tensor (N = 119 056: 24.7 ms -> see DESIGN.md).
// One 1024-thread workgroup per (head, query group) row.  The row's bf16 column sums are loaded ONCE into registers as
// order-preserving 16-bit keys (4 consecutive columns per thread per step, KPT/2 packed VGPRs), the k-th largest key is
// found by 16 rounds of bitwise bisection on block-wide counts (no sort, no histogram: the keys of one row sit in two or
// three exponent bins, a histogram's atomics would serialise), ties at the threshold are handed out in thread order,
// and the final mask bytes are written straight from the registers, 4 per thread per store.
struct TopkMaskParams {
    const uint16_t *cs;      // [rows, cs_stride] bf16
    const uint8_t *stat;     // optional static mask, row r -> stat + (r % stat_rows) * stat_stride
    const uint8_t *groups;   // optional per-row flag (the random / top-k part only applies where it is set)
    uint8_t *mask;           // [rows, n] bool bytes, fully overwritten
    int64_t cs_stride, stat_stride;
    int rows, n, k, stat_rows;
    float random_amount;
    uint32_t salt;           // per-launch value, see chipmunk_next_random_salt
    // PARTS form: row r of "cs" = bf16(sum of rows 3g .. 3g+2 of the partial rows of its (batch*head) block), g = r % groups
    const uint16_t *parts;
    int64_t pstride;         // elements between two partial rows
    int nrb, ngroups, nq;    // partial rows per (batch*head); 192-row groups per (batch*head); query rows
    // MASS form: k is the cap; a row keeps the smallest top set that carries top_p of its column-sum mass, at least k_min columns
    float top_p;
    int k_min;
    // padded batches (k_lens): rows [b * seq_rows, (b + 1) * seq_rows) belong to sequence b, whose columns >= klens[b] do not
    // exist -- they are read as the padding past n is (key 0), take part in no count, mass or tie, and their mask bytes are 0 whatever the
    // random part, the static mask and the group flag say.  nullptr: every row has n columns.
    const int32_t *klens;
    int seq_rows;
};

// valid columns of a row: n, or the row's sequence length clamped into [1, n]
__device__ __forceinline__ int topk_mask_row_len(const TopkMaskParams &p, int row) {
    if (!p.klens) return p.n;
    const int v = p.klens[row / p.seq_rows];
    return v < 1 ? 1 : (v < p.n ? v : p.n);
}
// ALIGNED forms: a row end nv that is no multiple of 4 falls inside ONE 4-column step of the row -- step (nv - 1) >> 12 of thread
// ((nv - 1) >> 2) & 1023 (thread t owns columns 4t + 4096j ..+3).  That step is loaded whole; these are the halves of its two words that
// belong to columns < nv (uniform over the workgroup, so the loops pay one compare per step and nothing per column).
struct RowCut {
    int tid, step;          // tid = -1: the row ends on a step boundary
    uint32_t keep0, keep1;
};
__device__ __forceinline__ RowCut row_cut(int nv) {
    const int rem = nv & 3;
    RowCut c;
    c.tid = rem ? ((nv - 1) >> 2) & 1023 : -1;
    c.step = (nv - 1) >> 12;
    c.keep0 = rem == 1 ? 0xffffu : 0xffffffffu;
    c.keep1 = rem == 3 ? 0xffffu : (rem ? 0u : 0xffffffffu);
    return c;
}

// ---- MASS (chipmunk_topk_mask_p): a per-row count in front of the selection.  The mass of a column is its bf16 value
// where that is positive (keys 0x8000 .. 0xff80), 0 otherwise (negative, NaN; also the padding past n, key 0).
//   total  = mass of the row,  target = float(top_p) * total                                                   (1 pass)
//   T      = the largest key with mass{key >= T} >= target: bits 14..0 below the fixed top bit, since all mass has key >= 0x8000
//            (15 passes; sums of a subset of non-negative terms in ONE fixed order are monotone in the subset, so this is a bisection)
//   k_p    = #{key > T} + min(#{key == T}, max(1, ceil((target - mass{key > T}) / value(T))))                   (1 pass)
//   k      = min(k, max(k_p, k_min)); k_p = 0 where total = 0.  The selection below then runs unchanged with this k.
// Every sum is fp32 in one fixed order: inside a thread its columns ascending, the 64 lanes of a wave by the xor tree
// (32, 16, .., 1: every lane ends with the same bits), then the 16 wave totals ascending.  Same launch, same bits.
// The value of a key >= 0x8000 is float((key ^ 0x8000) << 16); under that map a key below 0x8000 (a negative value) gives a negative number
// or a NaN, key 0 (the padding) gives -0.0, and a key above 0xff80 a NaN.  So "the key lies in [lo, 0xff80]" is ONE float compare,
// value >= value(lo): false for every NaN and every negative number, and the -0.0 it lets through at lo = 0x8000 adds nothing.
// A threshold above 0xff80 is a NaN itself: nothing passes, the mass is 0.
__device__ __forceinline__ float key_value(uint32_t key) { return __uint_as_float((key ^ 0x8000u) << 16); }
// both keys of a packed word, low column first, added to m
__device__ __forceinline__ void add_mass2(float &m, uint32_t kw, float flo) {
    const uint32_t kx = kw ^ 0x80008000u;
    const float a = __uint_as_float(kx << 16), b = __uint_as_float(kx & 0xffff0000u);
    m += a >= flo ? a : 0.f;
    m += b >= flo ? b : 0.f;
}

__device__ __forceinline__ int topp_count(float total, float target, float above, int gt, int eq, uint32_t thr, int k, int k_min) {
    int kp = 0;
    if (total > 0.f && target > 0.f) {
        const float v = key_value(thr);     // > 0: the keys equal to T carry the mass that reaches the target
        float t = __builtin_ceilf((target - above) / v);
        t = t >= 1.f ? t : 1.f;
        kp = gt + (t < (float)eq ? (int)t : eq);
    }
    const int s = kp > k_min ? kp : k_min;
    return s < k ? s : k;
}

__device__ __forceinline__ uint32_t bf16_key(uint32_t u) {  // monotone bf16 bits -> u16 (larger value = larger key)
    return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
}

template <int KPT, bool ALIGNED, bool PARTS = false, bool MASS = false>  // keys per thread (multiple of 4); the row must have n <= 1024 * KPT columns.
// PARTS (ALIGNED only): the row's column sums are not in memory; they are the sum of up to three bf16 partial rows (see above)
// MASS: the top-p count in front of the selection (see above); the values come back out of the key registers.
// ALIGNED: n % 4 == 0 and every row of cs / static mask / mask starts on an 8 / 4 / 4-byte boundary, so each thread
// step is one 8-byte load, one 4-byte load and one 4-byte store; the generic form goes element by element.
__global__ __launch_bounds__(1024) void topk_mask_kernel(const TopkMaskParams p) {
    constexpr int NV = KPT / 4;  // 4-column steps per thread
    __shared__ int wave_cnt[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = blockIdx.x;
    const int n = p.n;
    const int nv = topk_mask_row_len(p, row);   // the row's valid columns (k_lens), uniform over the workgroup
    const uint16_t *x = nullptr;
    int prow = 1;
    int64_t row1 = 0;      // PARTS: elements from the group's first partial row to its second
    if constexpr (PARTS) {
        const int bh = row / p.ngroups, g = row - bh * p.ngroups;
        int r0, r1;
        prow = colsum_part_rows(g, p.nrb / 2, r0, r1);
        x = p.parts + ((int64_t)bh * p.nrb + r0) * p.pstride;
        row1 = (int64_t)(r1 - r0) * p.pstride;
    } else {
        x = p.cs + (int64_t)row * p.cs_stride;
    }
    const uint32_t lane_off8 = 8u * (uint32_t)tid;    // byte offset of this thread's 4 bf16 inside a 4096-column step
    const uint32_t lane_off4 = 4u * (uint32_t)tid;    // ... of its 4 mask bytes
    // columns 4*tid + 4096*j .. +3; columns past n read as bf16 bits 0xffff = key 0, below every real key
    uint32_t key[NV][2];
    constexpr int LB = NV % 10 == 0 ? 10 : (NV % 8 == 0 ? 8 : (NV % 6 == 0 ? 6 : 4));  // loads in flight per batch
    static_assert(NV % LB == 0, "NV must split into whole load batches");
#pragma unroll
    for (int j0 = 0; j0 < NV; j0 += LB) {
        // batch of LB loads, then their conversion: bounds the live raw values (all NV at once would spill)
        uint32_t raw[LB][2];
#pragma unroll
        for (int jj = 0; jj < LB; ++jj) {
            const int c = 4 * tid + 4096 * (j0 + jj);
            uint32_t v0 = 0xffffffffu, v1 = 0xffffffffu;
            if constexpr (ALIGNED) {
                if (c < nv) {
                    // wave-uniform base + one shared 32-bit lane offset: the saddr form, no 64-bit address per step
                    const u32x2 v = *(const u32x2 *)((const unsigned char *)(x + 4096 * (j0 + jj)) + lane_off8);
                    v0 = v[0], v1 = v[1];
                    if constexpr (PARTS) {   // the combine, in its order: row 0 + row 1 in fp32, one rounding to bf16
                        if (prow == 2) {
                            float a0 = __uint_as_float(v0 << 16), a1 = __uint_as_float(v0 & 0xffff0000u);
                            float a2 = __uint_as_float(v1 << 16), a3 = __uint_as_float(v1 & 0xffff0000u);
                            const u32x2 y = *(const u32x2 *)((const unsigned char *)(x + row1 + 4096 * (j0 + jj)) + lane_off8);
                            a0 += __uint_as_float(y[0] << 16), a1 += __uint_as_float(y[0] & 0xffff0000u);
                            a2 += __uint_as_float(y[1] << 16), a3 += __uint_as_float(y[1] & 0xffff0000u);
                            v0 = pack_bf16x2(a0, a1), v1 = pack_bf16x2(a2, a3);
                        }
                    }
                }
            } else if (c < nv) {
                v0 = v1 = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t u = c + e < nv ? x[c + e] : 0xffffu;
                    if (e < 2) v0 |= u << (16 * e);
                    else v1 |= u << (16 * (e - 2));
                }
            }
            raw[jj][0] = v0, raw[jj][1] = v1;
        }
#pragma unroll
        for (int jj = 0; jj < LB; ++jj) {
            key[j0 + jj][0] = bf16_key(raw[jj][0] & 0xffffu) | (bf16_key(raw[jj][0] >> 16) << 16);
            key[j0 + jj][1] = bf16_key(raw[jj][1] & 0xffffu) | (bf16_key(raw[jj][1] >> 16) << 16);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (ALIGNED) {
        // k_lens: the step that straddles the row's end was loaded whole; its columns >= nv get key 0 like the rest of the padding
        const RowCut rc = row_cut(nv);
        if (tid == rc.tid) {
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (j == rc.step) key[j][0] &= rc.keep0, key[j][1] &= rc.keep1;
        }
    }
    auto block_count = [&](int mine) {  // sum over the 1024 threads, broadcast
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
        if (lane == 0) wave_cnt[w] = mine;
        __syncthreads();
        int t = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += wave_cnt[i];
        __syncthreads();
        return t;
    };
    const bool active = p.groups == nullptr || p.groups[row] != 0;
    int k = p.k < nv ? p.k : nv;
    if constexpr (MASS) {
        if (active && k > 0) {   // (uniform over the workgroup)
            // mass of the keys in [lo, 0xff80]: this thread's columns ascending, the wave's xor tree, the 16 wave totals ascending
            auto block_mass = [&](uint32_t lo) {
                const float flo = key_value(lo);
                float m = 0.f;
#pragma unroll
                for (int j = 0; j < NV; ++j)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        // add_mass2 spelled out: two temporaries per word and nothing hoisted out of the rounds (the KPT = 120 forms have
                        // 60 key registers of the 128 a 1024-thread workgroup gets; the compiler's own schedule of this loop spilled)
                        uint32_t t, a;
                        asm volatile("v_xor_b32 %1, 0x80008000, %3\n\t"
                                     "v_lshlrev_b32 %2, 16, %1\n\t"
                                     "v_and_b32 %1, 0xffff0000, %1\n\t"
                                     "v_cmp_ge_f32 vcc, %2, %4\n\t"
                                     "v_cndmask_b32 %2, 0, %2, vcc\n\t"
                                     "v_add_f32 %0, %0, %2\n\t"
                                     "v_cmp_ge_f32 vcc, %1, %4\n\t"
                                     "v_cndmask_b32 %1, 0, %1, vcc\n\t"
                                     "v_add_f32 %0, %0, %1"
                                     : "+v"(m), "=&v"(t), "=&v"(a)
                                     : "v"(key[j][h]), "s"(flo)
                                     : "vcc");
                    }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) m += __shfl_xor(m, d);
                if (lane == 0) wave_cnt[w] = __float_as_int(m);
                __syncthreads();
                float t = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) t += __int_as_float(wave_cnt[i]);
                __syncthreads();
                return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t)));   // (the same bits in every lane: scalar registers)
            };
            // ONE rolled loop around the unrolled pass (three copies of it cost registers): round 0 the total, rounds 1..15 the bisection
            // (a candidate above 0xff80 has mass 0 and is rejected), round 16 the mass above the threshold
            float total = 0.f, target = 0.f, above = 0.f;
            uint32_t res = 0x8000u;
#pragma nounroll
            for (int it = 0; it < 17; ++it) {
                const uint32_t lo = it == 0 ? 0x8000u : (it < 16 ? (res | (0x8000u >> it)) : res + 1u);
                const float m = block_mass(lo);
                if (it == 0) {
                    total = m, target = p.top_p * m;
                    if (!(total > 0.f && target > 0.f)) break;   // (uniform: every thread holds the same bits)
                } else if (it < 16) {
                    if (m >= target) res = lo;
                } else {
                    above = m;
                }
            }
            // #{key >= c} with the packed u16 counters of the selection's rounds below (three operations per two keys, nothing hoisted)
            auto count_ge = [&](uint32_t c) {
                const uint32_t cm1 = (c - 1u) | ((c - 1u) << 16), one2 = 0x00010001u;
                uint32_t cnt2 = 0;
#pragma unroll
                for (int j = 0; j < NV; ++j)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        uint32_t d;
                        asm volatile("v_pk_sub_u16 %0, %1, %2 clamp\n\tv_pk_min_u16 %0, %0, %3" : "=&v"(d) : "v"(key[j][h]), "v"(cm1), "v"(one2));
                        asm volatile("v_pk_add_u16 %0, %0, %1" : "+v"(cnt2) : "v"(d));
                    }
                return __builtin_amdgcn_readfirstlane(block_count((int)(cnt2 & 0xffffu) + (int)(cnt2 >> 16)));
            };
            const int gt = count_ge(res + 1u), eq = count_ge(res) - gt;     // (res <= 0xff80)
            k = topp_count(total, target, above, gt, eq, res, k, p.k_min);
        }
    }
    uint32_t thr = 0x10000u;  // keep nothing
    int ties_to_take = 0;
    if (active && k > 0) {
        // ---- largest T with #{key >= T} >= k, most significant bit first
        uint32_t res = 0;
        for (int bit = 15; bit >= 0; --bit) {
            const uint32_t cand = res | (1u << bit);
            // both 16-bit keys of a word at once: sat(key - (cand - 1)) is non-zero iff key >= cand; min(., 1) makes it a count;
            // packed u16 counters (a thread holds at most 4 * NV <= 480 keys).  Three VALU operations per two keys (the 32-bit
            // form took eight): this loop is 16 rounds x NV * 2 words x 16 waves on one CU's four SIMDs, the kernel's longest phase
            const uint32_t cm1 = (cand - 1u) | ((cand - 1u) << 16);
            const uint32_t one2 = 0x00010001u;
            uint32_t cnt2 = 0;
#pragma unroll
            for (int j = 0; j < NV; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    uint32_t d;
                    // (asm also keeps the optimiser from hoisting per-word work out of the 16 rounds)
                    asm volatile("v_pk_sub_u16 %0, %1, %2 clamp\n\tv_pk_min_u16 %0, %0, %3" : "=&v"(d) : "v"(key[j][h]), "v"(cm1), "v"(one2));
                    asm volatile("v_pk_add_u16 %0, %0, %1" : "+v"(cnt2) : "v"(d));
                }
            const int mine = (int)(cnt2 & 0xffffu) + (int)(cnt2 >> 16);
            if (block_count(mine) >= k) res = cand;
        }
        thr = res;
        int gt = 0;
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                uint32_t kw = key[j][h];
                asm volatile("" : "+v"(kw));
                gt += ((kw & 0xffffu) > thr ? 1 : 0) + ((kw >> 16) > thr ? 1 : 0);
            }
        ties_to_take = k - block_count(gt);  // >= 1 by construction of thr
    }
    // ---- ties at the threshold go to the lowest thread ids (torch.topk leaves the choice among equals unspecified)
    int my_ties = 0;
    if (ties_to_take > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                uint32_t kw = key[j][h];
                asm volatile("" : "+v"(kw));
                my_ties += ((kw & 0xffffu) == thr ? 1 : 0) + ((kw >> 16) == thr ? 1 : 0);
            }
    }
    int tie_budget = 0;
    {
        int incl = my_ties;  // inclusive scan over the block: wave scan, then the 16 wave totals
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wave_cnt[w] = incl;
        __syncthreads();
        int before = incl - my_ties;
#pragma unroll
        for (int i = 0; i < 16; ++i) before += i < w ? wave_cnt[i] : 0;
        __syncthreads();
        tie_budget = ties_to_take - before;  // how many of MY ties are taken (clamped below)
    }
    // ---- write the mask: (top-k | random) & group | static.  ROLLED loop that re-reads the row's column sums (the
    //      workgroup's own row: L2 / Infinity-Cache hits) instead of taking them from the key registers: an unrolled
    //      register-fed output loop needs ~60 more live registers than the selection and spilled at 30 steps per thread.
    uint8_t *out = p.mask + (int64_t)row * n;
    const uint8_t *st = p.stat ? p.stat + (int64_t)(row % p.stat_rows) * p.stat_stride : nullptr;
    const bool rnd = active && p.random_amount > 0.f;
    // (PARTS: the combined value at column c0..c0+3 again, same order of additions as in the selection pass)
    auto combined4 = [&](int c0, uint32_t &v0, uint32_t &v1) {
        const u32x2 v = *(const u32x2 *)(x + c0);
        v0 = v[0], v1 = v[1];
        if constexpr (PARTS) {
            float a0 = __uint_as_float(v0 << 16), a1 = __uint_as_float(v0 & 0xffff0000u);
            float a2 = __uint_as_float(v1 << 16), a3 = __uint_as_float(v1 & 0xffff0000u);
            if (prow == 2) {
                const u32x2 y = *(const u32x2 *)(x + row1 + c0);
                a0 += __uint_as_float(y[0] << 16), a1 += __uint_as_float(y[0] & 0xffff0000u);
                a2 += __uint_as_float(y[1] << 16), a3 += __uint_as_float(y[1] & 0xffff0000u);
            }
            v0 = pack_bf16x2(a0, a1), v1 = pack_bf16x2(a2, a3);
        }
    };
    uint32_t first = x[0];
    if constexpr (PARTS) {
        uint32_t f0, f1;
        combined4(0, f0, f1);
        first = f0 & 0xffffu;
    }
    const uint32_t salt = p.salt ^ (first * 0x27D4EB2Fu);
    const int nsteps = (n + 4095) / 4096;
    // keyed: v0 / v1 hold the order-preserving keys already (the selection's registers), else raw bf16 bits
    auto emit = [&](auto keyed, int c, uint32_t v0, uint32_t v1, uint32_t sb) {
        uint32_t bytes = 0;
        if constexpr (decltype(keyed)::value) asm volatile("" : "+v"(v0), "+v"(v1));   // opaque: no unpacking of all NV * 2 words ahead of time
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t half = ((e < 2 ? v0 : v1) >> (16 * (e & 1))) & 0xffffu;
            const uint32_t kv = decltype(keyed)::value ? half : bf16_key(half);
            bool keep = kv > thr;                      // thr = 0x10000 when the row is inactive or k = 0
            const bool tie = kv == thr && tie_budget > 0 && c + e < nv;
            tie_budget -= tie ? 1 : 0;
            keep = keep || tie;
            if (rnd && !keep) keep = hash_uniform(row, c + e, salt) < p.random_amount;
            keep = keep || ((sb >> (8 * e)) & 0xffu) != 0;
            keep = keep && c + e < nv;                 // (k_lens: no bit past the sequence's end, whatever set it)
            bytes |= (keep ? 1u : 0u) << (8 * e);
        }
        if constexpr (ALIGNED) {
            *(uint32_t *)(out + c) = bytes;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < n) out[c + e] = (uint8_t)(bytes >> (8 * e));
        }
    };
    if constexpr (ALIGNED) {
        // straight from the selection's key registers (no second pass over the column sums: with PARTS that was three rows again);
        // the static-mask words of OB steps are in flight together -- one workgroup per CU runs this kernel, so the loop's memory
        // parallelism is what a thread issues itself.  (Unrolled over all NV steps with the loads batched like this it stays under
        // the 128 registers of a 1024-thread workgroup; hoisting every load first is what spilled in round 2.)
        constexpr int OB = 5;
#pragma unroll
        for (int j0 = 0; j0 < NV; j0 += OB) {
            uint32_t sbv[OB];
#pragma unroll
            for (int jj = 0; jj < OB; ++jj) {
                const int c = 4 * tid + 4096 * (j0 + jj);
                sbv[jj] = (j0 + jj < NV && st && c < n) ? *(const uint32_t *)(st + c) : 0u;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int jj = 0; jj < OB; ++jj) {
                if constexpr (true) {
                    const int c = 4 * tid + 4096 * (j0 + jj);
                    if (j0 + jj < NV && c < n) emit(std::integral_constant<int, 1>{}, c, key[(j0 + jj) < NV ? (j0 + jj) : 0][0], key[(j0 + jj) < NV ? (j0 + jj) : 0][1], sbv[jj]);
                    asm volatile("" ::: "memory");   // one step's work at a time (the scheduler otherwise interleaves all NV and spills)
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        for (int j = 0; j < nsteps; ++j) {
            const int c = 4 * tid + 4096 * j;
            if (c >= n) break;
            uint32_t v0 = 0, v1 = 0, sb = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t u = c + e < nv ? x[c + e] : 0xffffu;
                if (e < 2) v0 |= u << (16 * e);
                else v1 |= u << (16 * (e - 2));
                if (st && c + e < n) sb |= (uint32_t)st[c + e] << (8 * e);
            }
            emit(std::integral_constant<int, 0>{}, c, v0, v1, sb);
        }
    }
}

// ---- the same selection for rows of any length up to CHIPMUNK_TOPK_MASK_MAX_N: the keys are not kept in registers, every
// bisection round STREAMS the row again (the workgroup's own row: 2 bytes per column, resident in this XCD's L2 after the first
// pass).  Same column-to-thread mapping as above (thread t owns columns 4t + 4096j + e), so counts, threshold, tie order
// (ascending thread, then ascending column) and therefore every mask bit are those of topk_mask_kernel.
// Passes over a row of n columns: [PARTS: 1 combine pass, 2-3 partial rows in (4-6n bytes, HBM), n keys out] + 16 bisection
// rounds + 1 pass counting keys above / at the threshold + 1 output pass = 18 reads of 2n bytes from L2, plus n static-mask
// bytes in and n mask bytes out.  Inactive rows and k = 0 skip all but the output pass, which then reads no keys either.
// PARTS: the three-row combine is done ONCE; its 16-bit keys are written over the group's first partial row (row r0 of
// colsum_part_rows belongs to that group alone, and the partial rows are scratch that nothing reads after this kernel), each
// thread over exactly the columns it read, and the later passes read keys (no conversion, one row instead of three).
// A thread counts at most 4 * 128 = 512 keys per round: two packed u16 counters of at most 256 each.
// (Key 0 is bf16 bits 0xffff, a NaN, and the padding past n: only with such a NaN at the threshold would padding enter a tie count.)
__device__ __forceinline__ uint32_t bf16_key2(uint32_t u) {   // bf16_key on both halves of a word
    uint32_t s;
    const uint32_t fifteen2 = 0x000f000fu;
    asm("v_pk_ashrrev_i16 %0, %1, %2" : "=v"(s) : "v"(fifteen2), "v"(u));   // 0xffff where the sign bit is set
    return u ^ (s | 0x80008000u);
}

// MASS: the top-p count (see key_value above) streams the row as well: 1 pass for the total, 15 bisection passes, 1 pass for the mass and
// count above the threshold and the count at it -- 17 more reads of the row's 2n bytes from L2 in front of the 18 of the selection.
template <bool ALIGNED, bool PARTS, bool MASS = false>
__global__ __launch_bounds__(1024) void topk_mask_stream_kernel(const TopkMaskParams p) {
    __shared__ int wave_cnt[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = blockIdx.x;
    const int n = p.n;
    const int nv = topk_mask_row_len(p, row);   // the row's valid columns (k_lens), uniform over the workgroup
    const uint16_t *x = nullptr;
    int prow = 1;
    int64_t row1 = 0;      // PARTS: elements from the group's first partial row to its second
    if constexpr (PARTS) {
        const int bh = row / p.ngroups, g = row - bh * p.ngroups;
        int r0, r1;
        prow = colsum_part_rows(g, p.nrb / 2, r0, r1);
        x = p.parts + ((int64_t)bh * p.nrb + r0) * p.pstride;
        row1 = (int64_t)(r1 - r0) * p.pstride;
    } else {
        x = p.cs + (int64_t)row * p.cs_stride;
    }
    const uint32_t lane_off8 = 8u * (uint32_t)tid;
    const int nsteps = (n + 4095) / 4096;
    const bool active = p.groups == nullptr || p.groups[row] != 0;
    int k = p.k < nv ? p.k : nv;
    const RowCut rc = row_cut(nv);
    const int cut_step = ALIGNED && tid == rc.tid ? rc.step : -1;   // k_lens: this thread's step that straddles the row's end, or none
    bool select = active && k > 0;
    const bool rnd = active && p.random_amount > 0.f;

    // (PARTS: the combined bf16 values of columns c0..c0+3, the additions in the order of the register form)
    auto combined4 = [&](int c0, uint32_t &v0, uint32_t &v1) {
        const u32x2 v = *(const u32x2 *)(x + c0);
        v0 = v[0], v1 = v[1];
        if constexpr (PARTS) {
            if (prow == 2) {
                float a0 = __uint_as_float(v0 << 16), a1 = __uint_as_float(v0 & 0xffff0000u);
                float a2 = __uint_as_float(v1 << 16), a3 = __uint_as_float(v1 & 0xffff0000u);
                const u32x2 y = *(const u32x2 *)(x + row1 + c0);
                a0 += __uint_as_float(y[0] << 16), a1 += __uint_as_float(y[0] & 0xffff0000u);
                a2 += __uint_as_float(y[1] << 16), a3 += __uint_as_float(y[1] & 0xffff0000u);
                v0 = pack_bf16x2(a0, a1), v1 = pack_bf16x2(a2, a3);
            }
        }
    };
    // the salt's row part, from the row's first (combined) element -- read before the keys overwrite it
    uint32_t first = 0;
    if (rnd) {
        first = x[0];
        if constexpr (PARTS) {
            uint32_t f0, f1;
            combined4(0, f0, f1);
            first = f0 & 0xffffu;
        }
    }
    const uint32_t salt = p.salt ^ (first * 0x27D4EB2Fu);
    if constexpr (PARTS) {
        __syncthreads();   // every thread has read column 0 before thread 0 replaces it
        if (select) {      // (uniform over the workgroup)
            uint16_t *xk = const_cast<uint16_t *>(x);
            for (int j = 0; j < nsteps; ++j) {
                const int c = 4 * tid + 4096 * j;
                if (c < nv) {   // (the partial rows hold nothing past the sequence's end: neither read nor written there)
                    uint32_t v0, v1;
                    combined4(c, v0, v1);
                    uint32_t k0 = bf16_key2(v0), k1 = bf16_key2(v1);
                    if (j == cut_step) k0 &= rc.keep0, k1 &= rc.keep1;   // key 0 for the columns >= nv of the straddling step
                    *(u32x2 *)(xk + c) = (u32x2){k0, k1};
                }
            }
        }
        __syncthreads();   // (a thread reads back only what it wrote itself; the barrier's wait drains the stores first)
    }
    // the keys of step j (columns 4 * tid + 4096 * j ..+3) as two packed words; columns past n have key 0, below every real key
    auto load_raw = [&](int j, uint32_t &v0, uint32_t &v1) {
        const int c = 4 * tid + 4096 * j;
        if constexpr (ALIGNED) {
            v0 = v1 = PARTS ? 0u : 0xffffffffu;
            if (c < nv) {
                const u32x2 v = *(const u32x2 *)((const unsigned char *)(x + 4096 * j) + lane_off8);
                v0 = v[0], v1 = v[1];
                if constexpr (!PARTS)
                    if (j == cut_step) v0 |= ~rc.keep0, v1 |= ~rc.keep1;   // raw 0xffff = key 0 (PARTS: cut when the keys were written)
            }
        } else {
            v0 = v1 = 0xffffffffu;
            if (c < nv) {
                v0 = v1 = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t u = c + e < nv ? x[c + e] : 0xffffu;
                    if (e < 2) v0 |= u << (16 * e);
                    else v1 |= u << (16 * (e - 2));
                }
            }
        }
    };
    auto to_keys = [&](uint32_t &v0, uint32_t &v1) {
        if constexpr (!PARTS) v0 = bf16_key2(v0), v1 = bf16_key2(v1);
    };
    auto block_count = [&](int mine) {  // sum over the 1024 threads, broadcast
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
        if (lane == 0) wave_cnt[w] = mine;
        __syncthreads();
        int t = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += wave_cnt[i];
        __syncthreads();
        return t;
    };
    constexpr int U = ALIGNED ? 8 : 2;   // row loads in flight per thread
    if constexpr (MASS) {
        if (select) {   // (uniform over the workgroup)
            // one pass: mass of the keys in [lo, 0xff80] (this thread's columns ascending, the wave's xor tree, the 16 wave totals
            // ascending) and, for the last pass, the keys above / at `lo - 1`
            auto block_mass = [&](uint32_t lo, int *gt, int *eq) {
                const float flo = key_value(lo);
                float m = 0.f;
                int g = 0, q = 0;
                for (int j0 = 0; j0 < nsteps; j0 += U) {
                    uint32_t kw[U][2];
#pragma unroll
                    for (int jj = 0; jj < U; ++jj) load_raw(j0 + jj, kw[jj][0], kw[jj][1]);
#pragma unroll
                    for (int jj = 0; jj < U; ++jj) {
                        to_keys(kw[jj][0], kw[jj][1]);
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const uint32_t lo16 = kw[jj][h] & 0xffffu, hi16 = kw[jj][h] >> 16;
                            add_mass2(m, kw[jj][h], flo);
                            if (gt) {
                                g += (lo16 >= lo ? 1 : 0) + (hi16 >= lo ? 1 : 0);
                                q += (lo16 == lo - 1u ? 1 : 0) + (hi16 == lo - 1u ? 1 : 0);
                            }
                        }
                    }
                }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) m += __shfl_xor(m, d);
                if (lane == 0) wave_cnt[w] = __float_as_int(m);
                __syncthreads();
                float t = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) t += __int_as_float(wave_cnt[i]);
                __syncthreads();
                if (gt) *gt = block_count(g), *eq = block_count(q);
                return t;
            };
            const float total = block_mass(0x8000u, nullptr, nullptr);
            const float target = p.top_p * total;
            uint32_t res = 0x8000u;
            if (total > 0.f && target > 0.f) {
                for (int bit = 14; bit >= 0; --bit) {
                    const uint32_t cand = res | (1u << bit);
                    if (cand > 0xff80u) continue;            // no mass up there (NaN keys)
                    if (block_mass(cand, nullptr, nullptr) >= target) res = cand;
                }
            }
            int gt = 0, eq = 0;
            // (res = 0xff80 = +inf outside the contract: the pass then sums keys in [0xff81, 0xff80], nothing, and counts the NaN keys)
            const float above = block_mass(res + 1u, &gt, &eq);
            k = topp_count(total, target, above, gt, eq, res, k, p.k_min);
            select = k > 0;
        }
    }
    uint32_t thr = 0x10000u;  // keep nothing
    int ties_to_take = 0, my_ties = 0;
    if (select) {
        // ---- largest T with #{key >= T} >= k, most significant bit first; one pass over the row per bit
        uint32_t res = 0;
        for (int bit = 15; bit >= 0; --bit) {
            const uint32_t cand = res | (1u << bit);
            const uint32_t cm1 = (cand - 1u) | ((cand - 1u) << 16);
            const uint32_t one2 = 0x00010001u;
            uint32_t cnt2 = 0;
            for (int j0 = 0; j0 < nsteps; j0 += U) {
                uint32_t kw[U][2];
#pragma unroll
                for (int jj = 0; jj < U; ++jj) load_raw(j0 + jj, kw[jj][0], kw[jj][1]);
#pragma unroll
                for (int jj = 0; jj < U; ++jj) {
                    to_keys(kw[jj][0], kw[jj][1]);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        uint32_t d;   // sat(key - (cand - 1)) is non-zero iff key >= cand; min(., 1) makes it a count (see above)
                        asm volatile("v_pk_sub_u16 %0, %1, %2 clamp\n\tv_pk_min_u16 %0, %0, %3" : "=&v"(d) : "v"(kw[jj][h]), "v"(cm1), "v"(one2));
                        asm volatile("v_pk_add_u16 %0, %0, %1" : "+v"(cnt2) : "v"(d));
                    }
                }
            }
            const int mine = (int)(cnt2 & 0xffffu) + (int)(cnt2 >> 16);
            if (block_count(mine) >= k) res = cand;
        }
        thr = res;
        // ---- keys above the threshold and keys at it, in one pass
        int gt = 0;
        for (int j0 = 0; j0 < nsteps; j0 += U) {
            uint32_t kw[U][2];
#pragma unroll
            for (int jj = 0; jj < U; ++jj) load_raw(j0 + jj, kw[jj][0], kw[jj][1]);
#pragma unroll
            for (int jj = 0; jj < U; ++jj) {
                to_keys(kw[jj][0], kw[jj][1]);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t lo = kw[jj][h] & 0xffffu, hi = kw[jj][h] >> 16;
                    gt += (lo > thr ? 1 : 0) + (hi > thr ? 1 : 0);
                    my_ties += (lo == thr ? 1 : 0) + (hi == thr ? 1 : 0);
                }
            }
        }
        ties_to_take = k - block_count(gt);  // >= 1 by construction of thr
    }
    // ---- ties at the threshold go to the lowest thread ids, inside a thread to its lowest columns
    int tie_budget = 0;
    {
        int incl = my_ties;  // inclusive scan over the block: wave scan, then the 16 wave totals
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wave_cnt[w] = incl;
        __syncthreads();
        int before = incl - my_ties;
#pragma unroll
        for (int i = 0; i < 16; ++i) before += i < w ? wave_cnt[i] : 0;
        __syncthreads();
        tie_budget = ties_to_take - before;  // how many of MY ties are taken (clamped below)
    }
    // ---- write the mask: (top-k | random) & group | static
    uint8_t *out = p.mask + (int64_t)row * n;
    const uint8_t *st = p.stat ? p.stat + (int64_t)(row % p.stat_rows) * p.stat_stride : nullptr;
    for (int j0 = 0; j0 < nsteps; j0 += U) {
        uint32_t kw[U][2], sbv[U];
#pragma unroll
        for (int jj = 0; jj < U; ++jj) {
            const int c = 4 * tid + 4096 * (j0 + jj);
            kw[jj][0] = kw[jj][1] = 0;
            if (select) load_raw(j0 + jj, kw[jj][0], kw[jj][1]);
            sbv[jj] = 0;
            if constexpr (ALIGNED) {
                if (st && c < n) sbv[jj] = *(const uint32_t *)(st + c);
            } else if (st) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < n) sbv[jj] |= (uint32_t)st[c + e] << (8 * e);
            }
        }
#pragma unroll
        for (int jj = 0; jj < U; ++jj) {
            const int c = 4 * tid + 4096 * (j0 + jj);
            if (c >= n) continue;
            if (select) to_keys(kw[jj][0], kw[jj][1]);
            uint32_t bytes = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t kv = (kw[jj][e >> 1] >> (16 * (e & 1))) & 0xffffu;
                bool keep = kv > thr;                      // thr = 0x10000 when the row is inactive or k = 0
                const bool tie = kv == thr && tie_budget > 0 && c + e < nv;
                tie_budget -= tie ? 1 : 0;
                keep = keep || tie;
                if (rnd && !keep) keep = hash_uniform(row, c + e, salt) < p.random_amount;
                keep = keep || ((sbv[jj] >> (8 * e)) & 0xffu) != 0;
                keep = keep && c + e < nv;                 // (k_lens: no bit past the sequence's end)
                bytes |= (keep ? 1u : 0u) << (8 * e);
            }
            if constexpr (ALIGNED) {
                *(uint32_t *)(out + c) = bytes;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < n) out[c + e] = (uint8_t)(bytes >> (8 * e));
            }
        }
    }
}

}  // namespace

extern "C" int chipmunk_mask_to_indices(const void *mask, int32_t *indices, int32_t *counts, int64_t rows, int n,
                                        int pad_n, int multiple_of, void *stream) {
    return launch_m2i<false>(mask, indices, counts, rows, n, pad_n, multiple_of, stream);
}

extern "C" int chipmunk_packed_mask_to_indices(const void *packed, int32_t *indices, int32_t *counts, int64_t rows,
                                               int n, int pad_n, int multiple_of, void *stream) {
    return launch_m2i<true>(packed, indices, counts, rows, n, pad_n, multiple_of, stream);
}

// the group forms (topk_group_delta_indices[_p]): the shape of the operands, checked here; the launch is launch_topk[_p]'s with one
// workgroup per (sequence, group)
struct TopkGroups {
    int batches, src_rows, group_rows;
    int groups() const { return (src_rows + group_rows - 1) / group_rows; }
};
static int check_topk_groups(const char *who, const TopkGroups &gs, const void *activation, const void *cache, const int32_t *indices,
                             const int32_t *counts, int cols, int *rows) {
    CM_CHECK(activation && cache && indices && counts, "%s: null pointer", who);
    CM_CHECK(cols >= 1024, "%s: cols >= 1024 required (the quantile is taken over the first 1024 columns); got cols=%d", who, cols);
    CM_CHECK(gs.group_rows >= 1 && gs.group_rows <= 64, "%s: rows_per_group must be in [1, 64] (got %d)", who, gs.group_rows);
    CM_CHECK(gs.batches >= 0 && gs.src_rows >= 1, "%s: B >= 0 and rows >= 1 required; got B=%d rows=%d", who, gs.batches, gs.src_rows);
    CM_CHECK((int64_t)gs.batches * gs.groups() < (1ll << 31), "%s: too many groups (B=%d times %d)", who, gs.batches, gs.groups());
    *rows = gs.batches * gs.groups();
    return CHIPMUNK_OK;
}

static int launch_topk(const void *activation, void *cache, int dtype, int32_t *indices, int32_t *counts, int rows,
                       int cols, double sparsity_amount, int multiple_of, double random_amount, void *stream,
                       const TopkGroups *gs = nullptr) {
    if (gs && check_topk_groups("topk_group_delta_indices", *gs, activation, cache, indices, counts, cols, &rows)) return CHIPMUNK_ERR_INVALID;
    CM_CHECK(activation && indices && counts, "topk_indices: null pointer");
    CM_CHECK(rows >= 0 && cols >= 1024, "topk_indices: rows >= 0 and cols >= 1024 required (the quantile is taken over the first 1024 columns); got rows=%d cols=%d", rows, cols);
    CM_CHECK(multiple_of > 0, "topk_indices: multiple_of must be positive");
    CM_CHECK(sparsity_amount >= 0.0 && sparsity_amount <= 1.0, "topk_indices: sparsity_amount must be in [0,1]");
    if (rows == 0) return CHIPMUNK_OK;
    TopkParams p = {activation, cache, indices, counts, rows, cols, multiple_of, (float)sparsity_amount, (float)random_amount,
                    random_amount > 0.0 ? chipmunk_next_random_salt() : 0u};
    if (gs) p.group_rows = gs->group_rows, p.src_rows = gs->src_rows, p.groups = gs->groups();
    hipStream_t s = (hipStream_t)stream;
#define LAUNCH_TOPK(T)                                                                                           \
    do {                                                                                                         \
        if (gs) hipLaunchKernelGGL((topk_indices_kernel<T, true, false, true>), dim3(rows), dim3(1024), 0, s, p); \
        else if (cache) hipLaunchKernelGGL((topk_indices_kernel<T, true>), dim3(rows), dim3(1024), 0, s, p);          \
        else hipLaunchKernelGGL((topk_indices_kernel<T, false>), dim3(rows), dim3(1024), 0, s, p);               \
    } while (0)
    switch (dtype) {
        case CHIPMUNK_DTYPE_BF16: LAUNCH_TOPK(uint16_t); break;
        case CHIPMUNK_DTYPE_FP16: LAUNCH_TOPK(_Float16); break;
        case CHIPMUNK_DTYPE_FP32: LAUNCH_TOPK(float); break;
        default: CM_CHECK(false, "topk_indices: unsupported dtype code %d", dtype);
    }
#undef LAUNCH_TOPK
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

// the _p forms: `who` names the entry point in the messages
static int launch_topk_p(const char *who, const void *activation, void *cache, int dtype, int32_t *indices, int32_t *counts, int rows,
                         int cols, double sparsity_amount, double top_p, double min_keys, int multiple_of, double random_amount,
                         void *stream, const TopkGroups *gs = nullptr) {
    if (gs && check_topk_groups(who, *gs, activation, cache, indices, counts, cols, &rows)) return CHIPMUNK_ERR_INVALID;
    CM_CHECK(activation && indices && counts, "%s: null pointer", who);
    CM_CHECK(rows >= 0 && cols >= 1024, "%s: rows >= 0 and cols >= 1024 required (the quantiles are taken over the first 1024 columns); got rows=%d cols=%d", who, rows, cols);
    CM_CHECK(multiple_of > 0, "%s: multiple_of must be positive", who);
    CM_CHECK(sparsity_amount >= 0.0 && sparsity_amount <= 1.0, "%s: sparsity_amount must be in [0,1]", who);
    CM_CHECK(top_p > 0.0 && top_p <= 1.0, "%s: top_p must be in (0, 1] (got %g)", who, top_p);
    // (1e-9: callers pass sparsity_amount = 1 - top_keys, and 1 - (1 - 0.1) is below 0.1 in double)
    CM_CHECK(min_keys >= 0.0 && min_keys <= 1.0 - sparsity_amount + 1e-9, "%s: min_keys must be in [0, 1 - sparsity_amount] (got %g with sparsity_amount %g)",
             who, min_keys, sparsity_amount);
    if (rows == 0) return CHIPMUNK_OK;
    TopkPParams p;
    p.act = activation, p.cache = cache, p.indices = indices, p.counts = counts;
    p.rows = rows, p.cols = cols, p.multiple_of = multiple_of;
    p.quantile = (float)sparsity_amount, p.random_amount = (float)random_amount;
    p.salt = random_amount > 0.0 ? chipmunk_next_random_salt() : 0u;
    p.top_p = (float)top_p;
    p.group_rows = gs ? gs->group_rows : 0, p.src_rows = gs ? gs->src_rows : 0, p.groups = gs ? gs->groups() : 0;
    // the floor's index in the sorted sample, never below the cap's (in exact arithmetic it is not): the kept set stays a subset of the cap's
    p.k_min = min_keys == 0.0 ? 1024 : std::max((int)(1024 * (float)(1.0 - min_keys)), (int)(1024 * p.quantile));
    hipStream_t s = (hipStream_t)stream;
#define LAUNCH_TOPK_P(T)                                                                                         \
    do {                                                                                                         \
        if (gs) hipLaunchKernelGGL((topk_indices_kernel<T, true, true, true>), dim3(rows), dim3(1024), 0, s, p); \
        else if (cache) hipLaunchKernelGGL((topk_indices_kernel<T, true, true>), dim3(rows), dim3(1024), 0, s, p);    \
        else hipLaunchKernelGGL((topk_indices_kernel<T, false, true>), dim3(rows), dim3(1024), 0, s, p);         \
    } while (0)
    switch (dtype) {
        case CHIPMUNK_DTYPE_BF16: LAUNCH_TOPK_P(uint16_t); break;
        case CHIPMUNK_DTYPE_FP16: LAUNCH_TOPK_P(_Float16); break;
        case CHIPMUNK_DTYPE_FP32: LAUNCH_TOPK_P(float); break;
        default: CM_CHECK(false, "%s: unsupported dtype code %d", who, dtype);
    }
#undef LAUNCH_TOPK_P
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

extern "C" int chipmunk_mask_to_sorted_indices(const void *mask, int packed, int32_t *indices, int32_t *counts,
                                               int64_t rows, int n, int pad_n, int multiple_of, void *stream) {
    return packed ? launch_m2i<true, true>(mask, indices, counts, rows, n, pad_n, multiple_of, stream)
                  : launch_m2i<false, true>(mask, indices, counts, rows, n, pad_n, multiple_of, stream);
}

extern "C" int chipmunk_mask_row_counts(const void *mask, int packed, int32_t *counts, int64_t *lengths, int64_t rows, int n,
                                        int pad_n, int multiple_of, void *stream) {
    CM_CHECK(mask && counts && lengths, "mask_row_counts: null pointer");
    CM_CHECK(rows >= 0 && n > 0 && pad_n >= n && multiple_of > 0, "mask_row_counts: bad sizes rows=%lld n=%d pad_n=%d multiple_of=%d",
             (long long)rows, n, pad_n, multiple_of);
    CM_CHECK(rows < (1ll << 31), "mask_row_counts: too many rows");
    CM_CHECK(!packed || n % 8 == 0, "mask_row_counts: n must be a multiple of 8 for a packed mask (got %d)", n);
    // this kernel uses no LDS; a row that neither emission order can take (the sorted one takes the longer rows) is refused here already
    const size_t lds = m2i_lds_bytes(n, true);
    CM_CHECK(lds <= 160 * 1024, "mask_to_indices: row length %d needs %zu B of LDS (> 160 KiB)", n, lds);
    if (rows == 0) return CHIPMUNK_OK;
    RowCountParams p = {(const uint8_t *)mask, counts, lengths, rows, n, pad_n, multiple_of};
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (packed) hipLaunchKernelGGL(mask_row_counts_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(mask_row_counts_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

extern "C" int chipmunk_mask_to_ragged_indices(const void *mask, int packed, int sorted, const int64_t *offsets, int32_t *flat,
                                               int64_t rows, int n, int multiple_of, void *stream) {
    if (packed) return sorted ? launch_m2i<true, true, true>(mask, flat, nullptr, rows, n, n, multiple_of, stream, offsets)
                              : launch_m2i<true, false, true>(mask, flat, nullptr, rows, n, n, multiple_of, stream, offsets);
    return sorted ? launch_m2i<false, true, true>(mask, flat, nullptr, rows, n, n, multiple_of, stream, offsets)
                  : launch_m2i<false, false, true>(mask, flat, nullptr, rows, n, n, multiple_of, stream, offsets);
}

extern "C" int chipmunk_topk_indices(const void *activation, int dtype, int32_t *indices, int32_t *counts, int rows,
                                     int cols, double sparsity_amount, int multiple_of, double random_amount,
                                     void *stream) {
    return launch_topk(activation, nullptr, dtype, indices, counts, rows, cols, sparsity_amount, multiple_of,
                       random_amount, stream);
}

extern "C" int chipmunk_topk_delta_indices(const void *activation, void *cache, int dtype, int32_t *indices,
                                           int32_t *counts, int rows, int cols, double sparsity_amount,
                                           int multiple_of, double random_amount, void *stream) {
    CM_CHECK(cache != nullptr, "topk_delta_indices: cache missing");
    return launch_topk(activation, cache, dtype, indices, counts, rows, cols, sparsity_amount, multiple_of,
                       random_amount, stream);
}

extern "C" int chipmunk_topk_indices_p(const void *activation, int dtype, int32_t *indices, int32_t *counts, int rows, int cols,
                                       double sparsity_amount, double top_p, double min_keys, int multiple_of,
                                       double random_amount, void *stream) {
    return launch_topk_p("topk_indices_p", activation, nullptr, dtype, indices, counts, rows, cols, sparsity_amount, top_p, min_keys,
                         multiple_of, random_amount, stream);
}

extern "C" int chipmunk_topk_delta_indices_p(const void *activation, void *cache, int dtype, int32_t *indices, int32_t *counts,
                                             int rows, int cols, double sparsity_amount, double top_p, double min_keys,
                                             int multiple_of, double random_amount, void *stream) {
    CM_CHECK(cache != nullptr, "topk_delta_indices_p: cache missing");
    return launch_topk_p("topk_delta_indices_p", activation, cache, dtype, indices, counts, rows, cols, sparsity_amount, top_p,
                         min_keys, multiple_of, random_amount, stream);
}

extern "C" int chipmunk_topk_group_delta_indices(const void *activation, void *cache, int dtype, int32_t *indices, int32_t *counts, int B,
                                                 int rows, int R, int cols, double sparsity_amount, int multiple_of,
                                                 double random_amount, void *stream) {
    const TopkGroups gs = {B, rows, R};
    return launch_topk(activation, cache, dtype, indices, counts, 0, cols, sparsity_amount, multiple_of, random_amount, stream, &gs);
}

extern "C" int chipmunk_topk_group_delta_indices_p(const void *activation, void *cache, int dtype, int32_t *indices, int32_t *counts,
                                                   int B, int rows, int R, int cols, double sparsity_amount, double top_p,
                                                   double min_keys, int multiple_of, double random_amount, void *stream) {
    const TopkGroups gs = {B, rows, R};
    return launch_topk_p("topk_group_delta_indices_p", activation, cache, dtype, indices, counts, 0, cols, sparsity_amount, top_p, min_keys,
                         multiple_of, random_amount, stream, &gs);
}

extern "C" int chipmunk_copy_indices(const void *src, void *dst, const int32_t *inds, const int32_t *counts, int B,
                                     int M, int R, int F, int elem_size, void *stream) {
    CM_CHECK(src && dst && inds && counts, "copy_indices: null pointer");
    CM_CHECK(B >= 0 && M > 0 && R > 0 && F > 0, "copy_indices: bad sizes");
    CM_CHECK(elem_size == 2 || elem_size == 4, "copy_indices: element size must be 2 or 4 bytes (got %d)", elem_size);
    const int64_t rows = (int64_t)B * M * R;
    if (rows == 0) return CHIPMUNK_OK;
    CM_CHECK(rows < (1ll << 31), "copy_indices: too many rows");
    hipStream_t s = (hipStream_t)stream;
    if (elem_size == 2)
        hipLaunchKernelGGL(copy_indices_kernel<uint16_t>, dim3((unsigned)rows), dim3(256), 0, s, (const uint16_t *)src,
                           (uint16_t *)dst, inds, counts, M, R, F);
    else
        hipLaunchKernelGGL(copy_indices_kernel<uint32_t>, dim3((unsigned)rows), dim3(256), 0, s, (const uint32_t *)src,
                           (uint32_t *)dst, inds, counts, M, R, F);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

extern "C" int chipmunk_bitpack(const void *mask, void *packed, int64_t n, void *stream) {
    CM_CHECK(mask && packed && n >= 0, "bitpack: bad arguments");
    if (n == 0) return CHIPMUNK_OK;
    const int64_t nb = (n + 7) >> 3;
    const unsigned grid = (unsigned)((nb + 255) / 256 < 8192 ? (nb + 255) / 256 : 8192);
    hipLaunchKernelGGL(bitpack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)mask,
                       (uint8_t *)packed, n);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

extern "C" int chipmunk_bitunpack(const void *packed, void *mask, int64_t n, void *stream) {
    CM_CHECK(mask && packed && n >= 0, "bitunpack: bad arguments");
    if (n == 0) return CHIPMUNK_OK;
    const int64_t nb = (n + 7) >> 3;
    const unsigned grid = (unsigned)((nb + 255) / 256 < 8192 ? (nb + 255) / 256 : 8192);
    hipLaunchKernelGGL(bitunpack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)packed,
                       (uint8_t *)mask, n);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

extern "C" int chipmunk_transpose16(const void *src, void *dst, int B, int R, int C, void *stream) {
    CM_CHECK(src && dst && B > 0 && R > 0 && C > 0, "transpose16: bad arguments");
    CM_CHECK((C & 7) == 0 || true, "unreachable");
    hipLaunchKernelGGL(transpose16_kernel, dim3((C + 63) / 64, (R + 63) / 64, B), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t *)src, (uint16_t *)dst, R, C, R);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

extern "C" int chipmunk_transpose16_pitched(const void *src, void *dst, int B, int R, int C, int ld, void *stream) {
    CM_CHECK(src && dst && B > 0 && R > 0 && C > 0, "transpose16: bad arguments");
    CM_CHECK(ld >= R, "transpose16: the output pitch ld (%d) must be at least R (%d)", ld, R);
    // the grid's row tiles cover [0, ld): the tiles past R hold zeros, which is what the padding gets
    hipLaunchKernelGGL(transpose16_kernel, dim3((C + 63) / 64, (ld + 63) / 64, B), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t *)src, (uint16_t *)dst, R, C, ld);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

// =====================================================================================  token reorder (row gather)
// The reference reorders tokens with einops / slicing chains under torch.compile (ops/patch.py:7-80: FLUX two-level
// patch order; ops/voxel.py:9-99: HunyuanVideo / Wan (4,6,8) voxel order with three tail regions, and their inverses).
// Every one of them is a fixed permutation of the token axis, so here it is ONE gather: dst[o, i, :] = src[o, map[i], :]
// with the permutation precomputed once per shape on the host side (chipmunk_amd/ops/_reorder.py) -- one pass at HBM
// rate instead of a reshape / permute / cat / index_put chain (HunyuanVideo: 118 800 rows of 6 KB per direction and step).
template <typename V>
__global__ __launch_bounds__(256) void gather_rows_kernel(const V *src, V *dst, const int32_t *map, int64_t n_out,
                                                          int64_t n_src, int64_t cpr, int64_t total) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t row = idx / cpr, c = idx - row * cpr;
        const int64_t o = row / n_out, r = row - o * n_out;
        dst[idx] = src[(o * n_src + map[r]) * cpr + c];
    }
}

extern "C" int chipmunk_gather_rows(const void *src, void *dst, const int32_t *map, int64_t outer, int64_t n_src,
                                    int64_t n_out, int64_t row_bytes, void *stream) {
    CM_CHECK(src && dst && map, "gather_rows: null pointer");
    CM_CHECK(outer >= 0 && n_src > 0 && n_out >= 0 && row_bytes > 0, "gather_rows: bad sizes");
    if (outer == 0 || n_out == 0) return CHIPMUNK_OK;
    hipStream_t s = (hipStream_t)stream;
    const uintptr_t align = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)row_bytes;
#define LAUNCH_GATHER(V)                                                                                              \
    do {                                                                                                              \
        const int64_t cpr = row_bytes / (int64_t)sizeof(V), total = outer * n_out * cpr;                               \
        const int64_t blocks = (total + 255) / 256;                                                                    \
        hipLaunchKernelGGL((gather_rows_kernel<V>), dim3((unsigned)(blocks > 65536 * 16 ? 65536 * 16 : blocks)),       \
                           dim3(256), 0, s, (const V *)src, (V *)dst, map, n_out, n_src, cpr, total);                  \
    } while (0)
    if ((align & 15) == 0) LAUNCH_GATHER(u32x4);
    else if ((align & 3) == 0) LAUNCH_GATHER(uint32_t);
    else if ((align & 1) == 0) LAUNCH_GATHER(uint16_t);
    else LAUNCH_GATHER(uint8_t);
#undef LAUNCH_GATHER
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

template <bool MASS>
static int topk_mask_parts_impl(const uint16_t *part, int part_stride, int nrb, int groups_per_bh, int Nq, const void *static_mask, int64_t static_stride,
                                int static_rows, const void *group_flags, void *mask, int rows, int n, int k, double random_amount,
                                double top_p, int k_min, hipStream_t s, const int32_t *klens, int seq_rows) {
    CM_CHECK(!klens || seq_rows > 0, "topk_mask_parts: k_lens without the rows per sequence");
    CM_CHECK(part && mask && rows >= 0 && n > 0 && (n & 3) == 0 && n <= CHIPMUNK_TOPK_MASK_MAX_N && k >= 0 && part_stride >= n && (part_stride & 3) == 0, "topk_mask_parts: bad arguments");
    CM_CHECK(!static_mask || (static_rows > 0 && static_stride >= n && (static_stride & 3) == 0 && ((uintptr_t)static_mask & 3) == 0),
             "topk_mask_parts: bad static mask geometry");
    CM_CHECK(((uintptr_t)mask & 3) == 0 && ((uintptr_t)part & 7) == 0, "topk_mask_parts: unaligned buffers");
    if (rows == 0) return CHIPMUNK_OK;
    TopkMaskParams p = {nullptr, (const uint8_t *)static_mask, (const uint8_t *)group_flags, (uint8_t *)mask, 0, static_stride,
                        rows, n, k, static_mask ? static_rows : 1, (float)random_amount,
                        random_amount > 0.0 ? chipmunk_next_random_salt() : 0u};
    p.parts = part, p.pstride = part_stride, p.nrb = nrb, p.ngroups = groups_per_bh, p.nq = Nq;
    p.top_p = (float)top_p, p.k_min = k_min;
    p.klens = klens, p.seq_rows = seq_rows;
    // rows past the register form's 122 880 columns (or option topk_mask_stream = 1: every row) take the streaming form
    if (n > 1024 * 120 || chipmunk_get_option("topk_mask_stream") == 1) hipLaunchKernelGGL((topk_mask_stream_kernel<true, true, MASS>), dim3(rows), dim3(1024), 0, s, p);
    else if (n <= 1024 * 16) hipLaunchKernelGGL((topk_mask_kernel<16, true, true, MASS>), dim3(rows), dim3(1024), 0, s, p);
    else if (n <= 1024 * 48) hipLaunchKernelGGL((topk_mask_kernel<48, true, true, MASS>), dim3(rows), dim3(1024), 0, s, p);
    else hipLaunchKernelGGL((topk_mask_kernel<120, true, true, MASS>), dim3(rows), dim3(1024), 0, s, p);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

int chipmunk_topk_mask_parts(const uint16_t *part, int part_stride, int nrb, int groups_per_bh, int Nq, const void *static_mask, int64_t static_stride,
                             int static_rows, const void *group_flags, void *mask, int rows, int n, int k, double random_amount,
                             hipStream_t s, const int32_t *klens, int seq_rows) {
    return topk_mask_parts_impl<false>(part, part_stride, nrb, groups_per_bh, Nq, static_mask, static_stride, static_rows, group_flags, mask, rows, n, k,
                                       random_amount, 0.0, 0, s, klens, seq_rows);
}

// the same with the top-p count in front (chipmunk_topk_mask_p): k is the cap
int chipmunk_topk_mask_p_parts(const uint16_t *part, int part_stride, int nrb, int groups_per_bh, int Nq, const void *static_mask, int64_t static_stride,
                               int static_rows, const void *group_flags, void *mask, int rows, int n, int k, double top_p, int k_min,
                               double random_amount, hipStream_t s, const int32_t *klens, int seq_rows) {
    CM_CHECK(top_p > 0.0 && top_p <= 1.0 && k_min >= 0, "topk_mask_p_parts: top_p must be in (0, 1] and k_min >= 0 (got %g, %d)", top_p, k_min);
    return topk_mask_parts_impl<true>(part, part_stride, nrb, groups_per_bh, Nq, static_mask, static_stride, static_rows, group_flags, mask, rows, n, k,
                                      random_amount, top_p, k_min, s, klens, seq_rows);
}

// ---- QKV projection output -> attention operands: split + q/k RMSNorm + head-major layout in ONE pass.
// The caller of the attention ops (reference examples/hunyuan/hyvideo/modules/models.py:188-193, 376-381) takes the projection's
// [n, 3*H*128] output apart with rearrange("B L (K H D) -> K B L H D"), applies RMSNorm over the head dimension to q and k
// (norm_layers.py:43-58: bf16(x_f32 * rsqrt(mean(x^2) + eps)) * weight, the product rounded to bf16 again) and transposes all
// three to the [B, H, n, 128] operands the kernels take -- two norm passes and three transposing copies in torch (8+ ms for the
// 2.2 GB of a HunyuanVideo layer).  Here: one 16-lane group per 256-byte (token, q|k|v, head) segment, 16 bytes per lane, the
// sum of squares by DPP inside the group; reads are contiguous over the projection's rows, writes are whole 256-byte rows.
// Optional rotary embedding of q and k (apply_rotary_emb, posemb_layers.py:133-172, the (cos, sin) form): for the first
// `rope_rows` tokens out = bf16(x_f32 * cos + rotate_half(x_f32) * sin), pairs (2i, 2i+1) -> (-x[2i+1], x[2i]); cos / sin fp32 [rope_rows, 128].
// A lane holds 8 consecutive elements = 4 whole pairs, so the rotation is lane-local.
__global__ __launch_bounds__(256) void qkv_split_norm_kernel(const uint16_t *qkv, int64_t row_stride, const uint16_t *qw,
                                                             const uint16_t *kw, uint16_t *q, uint16_t *k, uint16_t *v, int64_t n,
                                                             int H, float eps, int64_t segments, const float *fcos, const float *fsin,
                                                             int64_t rope_rows) {
    const int l15 = threadIdx.x & 15;
    u32x4 wq = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u}, wk = wq;   // bf16 1.0 pairs
    if (qw) wq = *(const u32x4 *)(qw + l15 * 8);
    if (kw) wk = *(const u32x4 *)(kw + l15 * 8);
    for (int64_t seg = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; seg < segments; seg += ((int64_t)gridDim.x * 256) >> 4) {
        const int64_t tok = seg / (3 * H);
        const int rem = (int)(seg - tok * 3 * H), which = rem / H, h = rem - which * H;
        u32x4 x = *(const u32x4 *)(qkv + tok * row_stride + (int64_t)rem * 128 + l15 * 8);
        uint16_t *dst = (which == 0 ? q : which == 1 ? k : v) + ((int64_t)h * n + tok) * 128 + l15 * 8;
        if (which < 2) {   // (uniform over the 16-lane group; the DPP row sum only mixes lanes of one group)
            float f[8], ss = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                f[2 * e] = __uint_as_float(x[e] << 16), f[2 * e + 1] = __uint_as_float(x[e] & 0xffff0000u);
                ss = __builtin_fmaf(f[2 * e], f[2 * e], ss);
                ss = __builtin_fmaf(f[2 * e + 1], f[2 * e + 1], ss);
            }
            ss = row16_sum(ss);
            const float r = 1.0f / __builtin_sqrtf(ss * (1.0f / 128.0f) + eps);   // (IEEE sqrt and divide, as torch.rsqrt on the host)
            const u32x4 w = which == 0 ? wq : wk;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = f[2 * e] * r, b = f[2 * e + 1] * r;
                round_bf16_pair(a, b);                                  // .type_as(x)
                x[e] = pack_bf16x2(a * __uint_as_float(w[e] << 16), b * __uint_as_float(w[e] & 0xffff0000u));   // * weight, in bf16
            }
            if (fcos && tok < rope_rows) {
                const f32x4 c0 = *(const f32x4 *)(fcos + tok * 128 + l15 * 8), c1 = *(const f32x4 *)(fcos + tok * 128 + l15 * 8 + 4);
                const f32x4 s0 = *(const f32x4 *)(fsin + tok * 128 + l15 * 8), s1 = *(const f32x4 *)(fsin + tok * 128 + l15 * 8 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float re = __uint_as_float(x[e] << 16), im = __uint_as_float(x[e] & 0xffff0000u);
                    const float cr = e < 2 ? c0[2 * e] : c1[2 * e - 4], ci = e < 2 ? c0[2 * e + 1] : c1[2 * e - 3];
                    const float sr = e < 2 ? s0[2 * e] : s1[2 * e - 4], si = e < 2 ? s0[2 * e + 1] : s1[2 * e - 3];
                    x[e] = pack_bf16x2(re * cr + (-im) * sr, im * ci + re * si);
                }
            }
        }
        *(u32x4 *)dst = x;
    }
}

extern "C" int chipmunk_qkv_split_norm(const void *qkv, int64_t row_stride, const void *q_weight, const void *k_weight, void *q,
                                       void *k, void *v, int64_t n, int heads, float eps, const float *freqs_cos,
                                       const float *freqs_sin, int64_t rope_rows, void *stream) {
    CM_CHECK(qkv && q && k && v, "qkv_split_norm: null pointer");
    CM_CHECK(n >= 0 && heads > 0 && row_stride >= (int64_t)3 * heads * 128, "qkv_split_norm: bad sizes");
    CM_CHECK((((uintptr_t)qkv | (uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)q_weight | (uintptr_t)k_weight) & 15) == 0 &&
                 (row_stride & 7) == 0 && (((uintptr_t)freqs_cos | (uintptr_t)freqs_sin) & 15) == 0,
             "qkv_split_norm: pointers and the row stride must be 16-byte aligned");
    CM_CHECK((freqs_cos == nullptr) == (freqs_sin == nullptr) && rope_rows >= 0 && rope_rows <= n, "qkv_split_norm: bad rotary arguments");
    if (n == 0) return CHIPMUNK_OK;
    const int64_t segments = n * 3 * heads, blocks = (segments + 15) / 16;
    hipLaunchKernelGGL(qkv_split_norm_kernel, dim3((unsigned)(blocks > 256 * 64 ? 256 * 64 : blocks)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t *)qkv, row_stride, (const uint16_t *)q_weight, (const uint16_t *)k_weight, (uint16_t *)q,
                       (uint16_t *)k, (uint16_t *)v, n, heads, eps, segments, freqs_cos, freqs_sin, freqs_cos ? rope_rows : 0);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

template <bool MASS>
static int topk_mask_impl(const void *cs, int64_t cs_stride, const void *static_mask, int64_t static_stride,
                          int static_rows, const void *group_flags, void *mask, int rows, int n, int k,
                          double random_amount, double top_p, int k_min, void *stream, const int32_t *klens = nullptr, int seq_rows = 0) {
    CM_CHECK(cs && mask, "topk_mask: null pointer");
    CM_CHECK(!klens || (seq_rows > 0 && rows % seq_rows == 0), "topk_mask: %d rows are no whole sequences of %d rows", rows, seq_rows);
    CM_CHECK(rows >= 0 && n > 0 && k >= 0, "topk_mask: bad sizes (rows=%d n=%d k=%d)", rows, n, k);
    CM_CHECK(cs_stride >= n, "topk_mask: cs row stride %lld < n %d", (long long)cs_stride, n);
    CM_CHECK(n <= CHIPMUNK_TOPK_MASK_MAX_N, "topk_mask: rows of more than %d columns are not supported (got %d)", CHIPMUNK_TOPK_MASK_MAX_N, n);
    CM_CHECK(!static_mask || (static_rows > 0 && static_stride >= n), "topk_mask: bad static mask geometry");
    CM_CHECK(random_amount >= 0.0 && random_amount <= 1.0, "topk_mask: random_amount must be in [0,1]");
    if (rows == 0) return CHIPMUNK_OK;
    TopkMaskParams p = {(const uint16_t *)cs, (const uint8_t *)static_mask, (const uint8_t *)group_flags, (uint8_t *)mask,
                        cs_stride, static_stride, rows, n, k, static_mask ? static_rows : 1, (float)random_amount,
                        random_amount > 0.0 ? chipmunk_next_random_salt() : 0u};
    p.top_p = (float)top_p, p.k_min = k_min;
    p.klens = klens, p.seq_rows = seq_rows;
    hipStream_t s = (hipStream_t)stream;
    const bool aligned = n % 4 == 0 && (((uintptr_t)cs) & 7) == 0 && (cs_stride * 2) % 8 == 0 && (((uintptr_t)mask) & 3) == 0 &&
                         (!static_mask || ((((uintptr_t)static_mask) & 3) == 0 && static_stride % 4 == 0));
#define LAUNCH_TM(KPT)                                                                                       \
    do {                                                                                                     \
        if (aligned) hipLaunchKernelGGL((topk_mask_kernel<KPT, true, false, MASS>), dim3(rows), dim3(1024), 0, s, p);     \
        else hipLaunchKernelGGL((topk_mask_kernel<KPT, false, false, MASS>), dim3(rows), dim3(1024), 0, s, p);            \
    } while (0)
    // rows past the register form's 122 880 columns (or option topk_mask_stream = 1: every row) take the streaming form
    if (n > 1024 * 120 || chipmunk_get_option("topk_mask_stream") == 1) {
        if (aligned) hipLaunchKernelGGL((topk_mask_stream_kernel<true, false, MASS>), dim3(rows), dim3(1024), 0, s, p);
        else hipLaunchKernelGGL((topk_mask_stream_kernel<false, false, MASS>), dim3(rows), dim3(1024), 0, s, p);
    } else if (n <= 1024 * 16) LAUNCH_TM(16);
    else if (n <= 1024 * 48) LAUNCH_TM(48);
    else LAUNCH_TM(120);
#undef LAUNCH_TM
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}

extern "C" int chipmunk_topk_mask(const void *cs, int64_t cs_stride, const void *static_mask, int64_t static_stride,
                                  int static_rows, const void *group_flags, void *mask, int rows, int n, int k,
                                  double random_amount, void *stream) {
    return topk_mask_impl<false>(cs, cs_stride, static_mask, static_stride, static_rows, group_flags, mask, rows, n, k, random_amount, 0.0, 0, stream);
}

extern "C" int chipmunk_topk_mask_p(const void *cs, int64_t cs_stride, const void *static_mask, int64_t static_stride,
                                    int static_rows, const void *group_flags, void *mask, int rows, int n, int k,
                                    double random_amount, double top_p, int k_min, void *stream) {
    CM_CHECK(top_p > 0.0 && top_p <= 1.0, "topk_mask_p: top_p must be in (0, 1] (got %g)", top_p);
    CM_CHECK(k_min >= 0, "topk_mask_p: k_min must be >= 0 (got %d)", k_min);
    return topk_mask_impl<true>(cs, cs_stride, static_mask, static_stride, static_rows, group_flags, mask, rows, n, k, random_amount, top_p, k_min, stream);
}

// The selection over a padded batch: k_lens = int32 [rows / seq_rows] on the device, rows [b * seq_rows, (b + 1) * seq_rows) belong to
// sequence b.  A row of sequence b selects among its first k_lens[b] columns only (k capped there) and writes 0 past them.
extern "C" int chipmunk_topk_mask_varlen(const void *cs, int64_t cs_stride, const void *static_mask, int64_t static_stride,
                                         int static_rows, const void *group_flags, void *mask, const int32_t *k_lens, int seq_rows, int rows,
                                         int n, int k, double random_amount, void *stream) {
    return topk_mask_impl<false>(cs, cs_stride, static_mask, static_stride, static_rows, group_flags, mask, rows, n, k, random_amount, 0.0, 0, stream,
                                 k_lens, seq_rows);
}

extern "C" int chipmunk_topk_mask_p_varlen(const void *cs, int64_t cs_stride, const void *static_mask, int64_t static_stride,
                                           int static_rows, const void *group_flags, void *mask, const int32_t *k_lens, int seq_rows, int rows,
                                           int n, int k, double random_amount, double top_p, int k_min, void *stream) {
    CM_CHECK(top_p > 0.0 && top_p <= 1.0, "topk_mask_p: top_p must be in (0, 1] (got %g)", top_p);
    CM_CHECK(k_min >= 0, "topk_mask_p: k_min must be >= 0 (got %d)", k_min);
    return topk_mask_impl<true>(cs, cs_stride, static_mask, static_stride, static_rows, group_flags, mask, rows, n, k, random_amount, top_p, k_min,
                                stream, k_lens, seq_rows);
}

extern "C" int chipmunk_compact_indices(const int32_t *indices, int64_t idx_stride, const int32_t *counts, const int64_t *offsets,
                                        int32_t *flat, int64_t rows, void *stream) {
    CM_CHECK(indices && counts && offsets && flat, "compact_indices: null pointer");
    CM_CHECK(rows >= 0 && rows < (1ll << 31) && idx_stride > 0, "compact_indices: bad sizes rows=%lld idx_stride=%lld", (long long)rows,
             (long long)idx_stride);
    if (rows == 0) return CHIPMUNK_OK;
    hipLaunchKernelGGL(compact_indices_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, indices, idx_stride, counts,
                       offsets, flat);
    CM_LAUNCH_CHECK();
    return CHIPMUNK_OK;
}
