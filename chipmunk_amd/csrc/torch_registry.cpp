// PyTorch operator registry over the C ABI (include/chipmunk_hip.h).
//
// Re-creates the reference's drop-in boundary: library `chipmunk` with byte-identical schemas and an importable
// extension module `cuda` whose load runs the static initialisers (reference csrc/chipmunk.cpp:9-25,45-80).
// ROCm PyTorch dispatches HIP tensors under the `CUDA` key, so FLUX / HunyuanVideo / Wan code written against
// `torch.ops.chipmunk.*` runs unchanged.  Every op enqueues on the CURRENT stream (the reference launches several
// ops on the legacy stream 0: csp_attn.cu:411, csp_mlp_mm1.cu:701, topk_indices.cu, mask_to_indices.cu:133).
// Argument checks mirror the reference's TORCH_CHECKs (file:line cited per op); failures raise c10::Error.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <Python.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <vector>

#include "../../include/chipmunk_hip.h"

extern "C" {
PyObject *PyInit_cuda(void) {
    static struct PyModuleDef module_def = {PyModuleDef_HEAD_INIT, "cuda", NULL, -1, NULL};
    return PyModule_Create(&module_def);
}
}

namespace chipmunk {
namespace {

void *cur_stream(const at::Tensor &t) {
    return (void *)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}
void check(int rc, const char *op) { TORCH_CHECK(rc == 0, "chipmunk::", op, ": ", chipmunk_last_error()); }

#define CHECK_DEV(x) TORCH_CHECK((x).is_cuda(), #x " must be a GPU tensor")
#define CHECK_BF16(x) TORCH_CHECK((x).scalar_type() == at::kBFloat16, #x " must be bfloat16")
#define CHECK_I32(x) TORCH_CHECK((x).scalar_type() == at::kInt, #x " must be a 32-bit integer tensor")
#define CHECK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")

struct Strides3 {
    int64_t s[3];
};
Strides3 strides_of(const at::Tensor &t, const char *name) {
    TORCH_CHECK(t.dim() == 4, name, " must be a 4D tensor [B,H,N,D]");
    TORCH_CHECK(t.size(3) == 128, "Head dimension must be 128");  // csp_attn.cu:381-383, dense_attn.cu:319-321
    TORCH_CHECK(t.stride(3) == 1, name, " must be contiguous in the head dimension");
    return {{t.stride(0), t.stride(1), t.stride(2)}};
}

void check_attn_shapes(const at::Tensor &q, const at::Tensor &k, const at::Tensor &v) {
    CHECK_DEV(q); CHECK_DEV(k); CHECK_DEV(v);
    CHECK_BF16(q); CHECK_BF16(k); CHECK_BF16(v);
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "q, k, v must be 4D tensors");
    TORCH_CHECK(k.size(0) == q.size(0) && v.size(0) == q.size(0), "batch dimension - idx 0 - must match for all inputs");
    TORCH_CHECK(k.size(1) == q.size(1) && v.size(1) == q.size(1), "QO heads must be equal to KV heads");
    TORCH_CHECK(v.size(2) == k.size(2), "K/V sequence length dimension - idx 2 - must match");
}

void check_indices(const at::Tensor &q, const at::Tensor &indices, const at::Tensor &counts, int64_t groups) {
    CHECK_DEV(indices); CHECK_DEV(counts);
    CHECK_CONTIG(indices); CHECK_CONTIG(counts);
    TORCH_CHECK(counts.dim() == 3, "Indices counts must be a 3D tensor");
    TORCH_CHECK(indices.dim() == 4, "Indices must be a 4D tensor");
    CHECK_I32(indices); CHECK_I32(counts);
    TORCH_CHECK(indices.size(0) == q.size(0) && counts.size(0) == q.size(0), "Indices batch dimension - idx 0 - must match for all inputs");
    TORCH_CHECK(indices.size(1) == q.size(1) && counts.size(1) == q.size(1), "Indices QO head dimension - idx 1 - must match for all inputs");
    TORCH_CHECK(indices.size(2) == groups && counts.size(2) == groups, "Indices query group dimension - idx 2 - must match for all inputs");
}

// ---------------------------------------------------------------------------------- attention
// reference csrc/attn/csp_attn.cu:315-423
void csp_attn(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor indices, at::Tensor indices_counts,
              int64_t o_scale) {
    check_attn_shapes(q, k, v);
    CHECK_DEV(o); CHECK_BF16(o);
    TORCH_CHECK(o_scale == 1 || o_scale == -1, "o_scale must be 1 or -1");
    TORCH_CHECK(o.sizes() == q.sizes(), "O must have the shape of Q");
    const int64_t groups = (q.size(2) + 191) / 192;
    check_indices(q, indices, indices_counts, groups);
    c10::DeviceGuard guard(q.device());
    auto qs = strides_of(q, "Q"), ks = strides_of(k, "K"), vs = strides_of(v, "V"), os = strides_of(o, "O");
    check(chipmunk_csp_attn(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), qs.s, ks.s, vs.s, os.s,
                            indices.data_ptr<int>(), indices_counts.data_ptr<int>(), (int)q.size(0), (int)q.size(1),
                            (int)q.size(2), (int)k.size(2), (int)indices.size(3), (int)o_scale, cur_stream(q)),
          "csp_attn");
}

// addition: o_in + o_scale * sparse attention into a fresh tensor (the clone + in-place pair of modules/attn.py:186-188)
at::Tensor csp_attn_out(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o_in, at::Tensor indices,
                        at::Tensor indices_counts, int64_t o_scale) {
    check_attn_shapes(q, k, v);
    CHECK_DEV(o_in); CHECK_BF16(o_in);
    TORCH_CHECK(o_scale == 1 || o_scale == -1, "o_scale must be 1 or -1");
    TORCH_CHECK(o_in.sizes() == q.sizes(), "O must have the shape of Q");
    const int64_t groups = (q.size(2) + 191) / 192;
    check_indices(q, indices, indices_counts, groups);
    c10::DeviceGuard guard(q.device());
    // the result takes o_in's layout when that has contiguous 128-element rows (e.g. the token-major cache of a dense call with
    // token_major_o): o_in and o share one set of strides in the C entry
    const bool keep = o_in.stride(3) == 1 && o_in.is_non_overlapping_and_dense();
    at::Tensor oi = keep ? o_in : o_in.contiguous();
    at::Tensor o = at::empty_strided(oi.sizes(), oi.strides(), oi.options());
    auto qs = strides_of(q, "Q"), ks = strides_of(k, "K"), vs = strides_of(v, "V"), os = strides_of(o, "O");
    check(chipmunk_csp_attn_out(q.data_ptr(), k.data_ptr(), v.data_ptr(), oi.data_ptr(), o.data_ptr(), qs.s, ks.s, vs.s,
                                os.s, indices.data_ptr<int>(), indices_counts.data_ptr<int>(), (int)q.size(0),
                                (int)q.size(1), (int)q.size(2), (int)k.size(2), (int)indices.size(3), (int)o_scale,
                                cur_stream(q)),
          "csp_attn_out");
    return o;
}

// addition: padded index rows [B,H,G,W] + counts -> (flat int32 rows back to back, int64 offsets [B*H*G + 1]); every row is
// rounded up to 32 entries (zero filled) so that whole key tiles can be read, 64 spare entries at the end
std::vector<at::Tensor> compact_indices(at::Tensor indices, at::Tensor counts) {
    CHECK_DEV(indices); CHECK_DEV(counts); CHECK_I32(indices); CHECK_I32(counts); CHECK_CONTIG(indices); CHECK_CONTIG(counts);
    TORCH_CHECK(indices.dim() == 4 && counts.dim() == 3 && indices.size(0) == counts.size(0) && indices.size(1) == counts.size(1) &&
                indices.size(2) == counts.size(2), "indices must be [B,H,G,W] and counts [B,H,G]");
    c10::DeviceGuard guard(indices.device());
    const int64_t rows = counts.numel(), W = indices.size(3);
    at::Tensor len = counts.flatten().clamp(0, W).to(at::kLong).add_(31).div_(32, "floor").mul_(32);
    at::Tensor offsets = at::zeros({rows + 1}, len.options());
    if (rows) offsets.narrow(0, 1, rows).copy_(len.cumsum(0));
    const int64_t total = rows ? offsets[rows].item<int64_t>() : 0;      // one host sync (a mask-recompute step, not the sparse step)
    at::Tensor flat = at::empty({total + 64}, indices.options());
    flat.narrow(0, total, 64).zero_();
    check(chipmunk_compact_indices(indices.data_ptr<int>(), W, counts.data_ptr<int>(), offsets.data_ptr<int64_t>(), flat.data_ptr<int>(),
                                   rows, cur_stream(indices)),
          "compact_indices");
    return {flat, offsets};
}

// addition: csp_attn_out over the ragged rows of compact_indices
at::Tensor csp_attn_out_ragged(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o_in, at::Tensor indices, at::Tensor offsets,
                               at::Tensor indices_counts, int64_t o_scale) {
    check_attn_shapes(q, k, v);
    CHECK_DEV(o_in); CHECK_BF16(o_in); CHECK_DEV(indices); CHECK_DEV(offsets); CHECK_DEV(indices_counts);
    CHECK_I32(indices); CHECK_I32(indices_counts); CHECK_CONTIG(indices); CHECK_CONTIG(offsets); CHECK_CONTIG(indices_counts);
    TORCH_CHECK(offsets.scalar_type() == at::kLong, "offsets must be int64");
    TORCH_CHECK(o_scale == 1 || o_scale == -1, "o_scale must be 1 or -1");
    TORCH_CHECK(o_in.sizes() == q.sizes(), "O must have the shape of Q");
    const int64_t groups = (q.size(2) + 191) / 192;
    TORCH_CHECK(indices_counts.dim() == 3 && indices_counts.size(0) == q.size(0) && indices_counts.size(1) == q.size(1) &&
                indices_counts.size(2) == groups, "counts must be [B, H, ceil(N/192)]");
    TORCH_CHECK(offsets.numel() == indices_counts.numel() + 1, "offsets must have one entry per (batch, head, group) + 1");
    c10::DeviceGuard guard(q.device());
    const bool keep = o_in.stride(3) == 1 && o_in.is_non_overlapping_and_dense();
    at::Tensor oi = keep ? o_in : o_in.contiguous();
    at::Tensor o = at::empty_strided(oi.sizes(), oi.strides(), oi.options());
    auto qs = strides_of(q, "Q"), ks = strides_of(k, "K"), vs = strides_of(v, "V"), os = strides_of(o, "O");
    check(chipmunk_csp_attn_out_ragged(q.data_ptr(), k.data_ptr(), v.data_ptr(), oi.data_ptr(), o.data_ptr(), qs.s, ks.s, vs.s, os.s,
                                       indices.data_ptr<int>(), offsets.data_ptr<int64_t>(), indices_counts.data_ptr<int>(),
                                       (int)q.size(0), (int)q.size(1), (int)q.size(2), (int)k.size(2), (int)o_scale, cur_stream(q)),
          "csp_attn_out_ragged");
    return o;
}

// addition (model code in the reference): x + gate * y -> LayerNorm -> * (1 + scale) + shift in one pass; returns {x_out, xm};
// without y / gate: {x, xm}
std::vector<at::Tensor> residual_ln_modulate(at::Tensor x, const c10::optional<at::Tensor> &y, const c10::optional<at::Tensor> &gate,
                                             at::Tensor shift, at::Tensor scale, double eps) {
    CHECK_DEV(x); CHECK_BF16(x); CHECK_CONTIG(x); CHECK_DEV(shift); CHECK_BF16(shift); CHECK_DEV(scale); CHECK_BF16(scale);
    TORCH_CHECK(x.dim() >= 2, "x must be [..., rows, cols]");
    const int64_t C = x.size(-1), rows = x.numel() / C;
    const bool res = y.has_value() && y->defined();
    TORCH_CHECK(res == (gate.has_value() && gate->defined()), "y and gate come together");
    at::Tensor sh = shift.contiguous(), sc = scale.contiguous(), yc, gc, xo;
    TORCH_CHECK(sh.numel() == C && sc.numel() == C, "shift / scale must have one entry per column");
    if (res) {
        yc = *y; gc = gate->contiguous();
        CHECK_DEV(yc); CHECK_BF16(yc); CHECK_CONTIG(yc); CHECK_DEV(gc); CHECK_BF16(gc);
        TORCH_CHECK(yc.sizes() == x.sizes() && gc.numel() == C, "y must have the shape of x, gate one entry per column");
        xo = at::empty_like(x);
    }
    c10::DeviceGuard guard(x.device());
    at::Tensor xm = at::empty_like(x);
    check(chipmunk_residual_ln_modulate(x.data_ptr(), res ? yc.data_ptr() : nullptr, res ? gc.data_ptr() : nullptr, sh.data_ptr(),
                                        sc.data_ptr(), res ? xo.data_ptr() : nullptr, xm.data_ptr(), rows, (int)C, eps, cur_stream(x)),
          "residual_ln_modulate");
    // without a residual the input is not handed back: an operator's outputs must not alias its inputs (the schema declares fresh
    // tensors; functionalisation / torch.compile rely on it) -- the Python wrapper returns the caller's x beside xm
    if (res) return {xo, xm};
    return {xm};
}

// addition (Wan's block glue, model code in the reference: examples/wan/wan/modules/model.py:100-110, 317-334): fp32 residual stream,
// fp32 vectors per sequence ([C], [B, C] or [B, 1, C]), modulation (shift, scale) or affine (weight, bias); returns {x_out fp32, xm bf16}
// with y, {xm} without (the Python wrapper hands the caller's x back: an operator's outputs never alias its inputs)
std::vector<at::Tensor> residual_ln_modulate_f32(at::Tensor x, const c10::optional<at::Tensor> &y, const c10::optional<at::Tensor> &gate,
                                                 const c10::optional<at::Tensor> &shift, const c10::optional<at::Tensor> &scale,
                                                 const c10::optional<at::Tensor> &weight, const c10::optional<at::Tensor> &bias, double eps) {
    auto has = [](const c10::optional<at::Tensor> &t) { return t.has_value() && t->defined(); };
    CHECK_DEV(x); CHECK_CONTIG(x);
    TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "x must be float32 or bfloat16");
    TORCH_CHECK(x.dim() == 2 || x.dim() == 3, "x must be [B, L, C] or [L, C]");
    const int64_t C = x.size(-1), L = x.size(-2), B = x.dim() == 3 ? x.size(0) : 1;
    TORCH_CHECK(B >= 1 && C >= 1, "x must not be empty in its batch or column dimension");
    const bool res = has(y), mod = has(shift) || has(scale), aff = has(weight) || has(bias);
    TORCH_CHECK(has(shift) == has(scale) && has(weight) == has(bias), "shift / scale come together, and so do weight / bias");
    TORCH_CHECK(mod != aff, "exactly one of modulation (shift, scale) and affine (weight, bias)");
    TORCH_CHECK(res || !has(gate), "a gate without y");
    TORCH_CHECK(!(res && !has(gate) && x.scalar_type() == at::kBFloat16), "a bfloat16 x takes its residual with a gate");
    // a vector per sequence: fp32 [C], [B, C] or [B, 1, C] -> (contiguous tensor, batch stride in elements)
    auto vec = [&](const at::Tensor &t, const char *name, int64_t &stride) {
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat, name, " must be a float32 GPU tensor");
        const bool one = t.dim() == 1 && t.size(0) == C;
        const bool per = (t.dim() == 2 && t.size(1) == C) || (t.dim() == 3 && t.size(1) == 1 && t.size(2) == C);
        TORCH_CHECK(one || (per && (t.size(0) == 1 || t.size(0) == B)), name, " must be [C], [B, C] or [B, 1, C] with a batch dimension of 1 or B");
        stride = (per && t.size(0) == B && B > 1) ? C : 0;
        return t.contiguous();
    };
    at::Tensor yc, gc, sh, sc, wt, bs, xo;
    int64_t gs = 0, ms = 0, ms2 = 0, none = 0;
    if (res) {
        yc = *y;
        CHECK_DEV(yc); CHECK_BF16(yc); CHECK_CONTIG(yc);
        TORCH_CHECK(yc.sizes() == x.sizes(), "y must have the shape of x");
        if (has(gate)) gc = vec(*gate, "gate", gs);
    }
    if (mod) {
        sh = vec(*shift, "shift", ms), sc = vec(*scale, "scale", ms2);
        if (ms != ms2) {   // one of the two is a single vector: give both the batch stride
            if (ms == 0) sh = sh.reshape({1, C}).expand({B, C}).contiguous();
            else sc = sc.reshape({1, C}).expand({B, C}).contiguous();
            ms = C;
        }
    } else {
        TORCH_CHECK(weight->dim() == 1 && bias->dim() == 1, "weight / bias must be [C]");
        wt = vec(weight->to(at::kFloat), "weight", none), bs = vec(bias->to(at::kFloat), "bias", none);   // widening is exact
    }
    c10::DeviceGuard guard(x.device());
    if (res) xo = at::empty(x.sizes(), x.options().dtype(at::kFloat));
    at::Tensor xm = at::empty(x.sizes(), x.options().dtype(at::kBFloat16));
    check(chipmunk_residual_ln_modulate_f32(x.data_ptr(), x.scalar_type() == at::kBFloat16 ? 1 : 2, res ? yc.data_ptr() : nullptr,
                                            gc.defined() ? gc.data_ptr<float>() : nullptr, gs, mod ? sh.data_ptr<float>() : nullptr,
                                            mod ? sc.data_ptr<float>() : nullptr, ms, mod ? nullptr : wt.data_ptr<float>(),
                                            mod ? nullptr : bs.data_ptr<float>(), res ? xo.data_ptr<float>() : nullptr, xm.data_ptr(), B, L,
                                            (int)C, eps, cur_stream(x)),
          "residual_ln_modulate_f32");
    if (res) return {xo, xm};
    return {xm};
}

// reference csrc/attn/csp_128_attn.cu:355-461
at::Tensor csp_128_attn(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor indices, at::Tensor indices_counts) {
    check_attn_shapes(q, k, v);
    TORCH_CHECK(q.is_contiguous(), "Q must be contiguous");
    TORCH_CHECK(k.is_contiguous(), "K must be contiguous");
    TORCH_CHECK(v.is_contiguous(), "V must be contiguous");
    TORCH_CHECK(q.size(3) == 128, "Head dimension must be 128");
    // The reference additionally demands seq_len % 192 == 0 and indices.size(3) == seq_len (csp_128_attn.cu:419,429)
    // and its Python wrapper pads q / indices to get there (ops/attn.py:146-161).  The gfx950 kernel masks the ragged
    // last group itself, so both are accepted as-is (a superset of the reference's valid inputs).
    const int64_t groups = (q.size(2) + 191) / 192;
    check_indices(q, indices, indices_counts, groups);
    c10::DeviceGuard guard(q.device());
    at::Tensor o = at::empty(q.sizes(), v.options());
    check(chipmunk_csp_128_attn(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), indices.data_ptr<int>(),
                                indices_counts.data_ptr<int>(), (int)q.size(0), (int)q.size(1), (int)q.size(2),
                                (int)k.size(2), (int)indices.size(3), cur_stream(q)),
          "csp_128_attn");
    return o;
}

// [B, H, N, 128] output of the dense operators: contiguous as the reference's, or (token_major_o, an addition) the permuted view
// of [B, N, H, 128] storage, which `o.permute(0, 2, 1, 3).reshape(B, N, H * 128)` turns into the next GEMM's operand for free
static at::Tensor alloc_o(const at::Tensor &q, const at::Tensor &v, bool token_major) {
    if (!token_major) return at::empty(q.sizes(), v.options().memory_format(at::MemoryFormat::Contiguous));
    return at::empty({q.size(0), q.size(2), q.size(1), q.size(3)}, v.options()).permute({0, 2, 1, 3});
}

// per-sequence key lengths of a padded batch (an addition): int32 [B] on the GPU; nullptr when absent
using OptTensor = c10::optional<at::Tensor>;
static const int32_t *klens_ptr(const OptTensor &k_lens, const at::Tensor &like, int64_t B) {
    if (!k_lens.has_value() || !k_lens->defined()) return nullptr;
    const at::Tensor &t = *k_lens;
    TORCH_CHECK(t.is_cuda() && t.device() == like.device(), "k_lens must be a GPU tensor on the device of the other operands");
    TORCH_CHECK(t.scalar_type() == at::kInt, "k_lens must be int32");
    TORCH_CHECK(t.is_contiguous() && t.numel() == B, "k_lens must be contiguous with one entry per sequence (", B, "), got ", t.numel());
    return t.data_ptr<int32_t>();
}

// reference csrc/attn/dense_attn.cu:246-372
static std::vector<at::Tensor> dense_attn_klens(at::Tensor q, at::Tensor k, at::Tensor v, bool token_major_o, const OptTensor &k_lens) {
    check_attn_shapes(q, k, v);
    const int32_t *kl = klens_ptr(k_lens, q, q.size(0));
    c10::DeviceGuard guard(q.device());
    auto qs = strides_of(q, "Q"), ks = strides_of(k, "K"), vs = strides_of(v, "V");
    at::Tensor o = alloc_o(q, v, token_major_o);
    auto os = strides_of(o, "O");
    at::Tensor l = at::empty({q.size(0), q.size(1), q.size(2), 1}, q.options().dtype(at::kFloat));
    check(chipmunk_dense_attn_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), qs.s, ks.s, vs.s, o.data_ptr(), os.s,
                                     l.data_ptr<float>(), kl, (int)q.size(0), (int)q.size(1), (int)q.size(2), (int)k.size(2),
                                     cur_stream(q)),
          "dense_attn");
    return {o, l};
}

std::vector<at::Tensor> dense_attn_layout(at::Tensor q, at::Tensor k, at::Tensor v, bool token_major_o) {
    return dense_attn_klens(q, k, v, token_major_o, c10::nullopt);
}
std::vector<at::Tensor> dense_attn_varlen(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor k_lens, bool token_major_o) {
    return dense_attn_klens(q, k, v, token_major_o, k_lens);
}

std::vector<at::Tensor> dense_attn(at::Tensor q, at::Tensor k, at::Tensor v) { return dense_attn_layout(q, k, v, false); }

// reference csrc/attn/dense_colsum_attn.cu:521-668
static std::vector<at::Tensor> dense_colsum_attn_klens(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor p, bool token_major_o,
                                                       const OptTensor &k_lens) {
    check_attn_shapes(q, k, v);
    const int32_t *kl = klens_ptr(k_lens, q, q.size(0));
    CHECK_DEV(p);
    TORCH_CHECK(p.scalar_type() == at::kFloat, "p must be float32");
    TORCH_CHECK(p.is_contiguous(), "p must be contiguous");
    TORCH_CHECK(p.numel() == q.size(0) * q.size(1) * q.size(2), "p must have one entry per query row [B,H,N,1]");
    c10::DeviceGuard guard(q.device());
    auto qs = strides_of(q, "Q"), ks = strides_of(k, "K"), vs = strides_of(v, "V");
    const int64_t groups = (q.size(2) + 191) / 192;
    // the reference's cs has one column per (padded) query position (:580-583: it only ever sees Nk <= Nq); a rank that holds a
    // slice of the query rows against the whole sequence's keys (query-group sharding) gets one column per key
    const int64_t width = std::max<int64_t>(q.size(2), k.size(2));
    at::Tensor o = alloc_o(q, v, token_major_o);
    auto os = strides_of(o, "O");
    at::Tensor cs = at::empty({q.size(0), q.size(1), groups, width}, v.options());
    at::Tensor l = at::empty({q.size(0), q.size(1), q.size(2), 1}, q.options().dtype(at::kFloat));
    check(chipmunk_dense_colsum_attn_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), qs.s, ks.s, vs.s, p.data_ptr<float>(),
                                            o.data_ptr(), os.s, cs.data_ptr(), l.data_ptr<float>(), kl, (int)q.size(0),
                                            (int)q.size(1), (int)q.size(2), (int)k.size(2), (int)width, cur_stream(q)),
          "dense_colsum_attn");
    return {o, cs, l};
}

std::vector<at::Tensor> dense_colsum_attn_layout(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor p, bool token_major_o) {
    return dense_colsum_attn_klens(q, k, v, p, token_major_o, c10::nullopt);
}
std::vector<at::Tensor> dense_colsum_attn_varlen(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor p, at::Tensor k_lens, bool token_major_o) {
    return dense_colsum_attn_klens(q, k, v, p, token_major_o, k_lens);
}

std::vector<at::Tensor> dense_colsum_attn(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor p) {
    return dense_colsum_attn_layout(q, k, v, p, false);
}

// ---------------------------------------------------------------------------------- MLP
// The column-major activation cache as the MLP operators take it: [F, M] (leading dimensions of size 1 allowed), elements of a column
// contiguous, columns `ldc` elements apart -- a contiguous tensor (ldc = M) or the [:, :M] view of a buffer with padded columns.
// M % 128 == 0 with ldc == M goes to the reference's entry points, everything else to the *_ragged ones (include/chipmunk_hip.h).
int64_t cache_pitch(const at::Tensor &t, int64_t F, int64_t M, const char *name) {
    // (a group-major cache [G, F, 128] of whole groups has the F * M elements of the column-major one: it is told apart by its shape)
    TORCH_CHECK(!(M > 128 && t.dim() >= 3 && t.size(-1) == 128 && t.size(-2) == F && t.size(-3) * 128 == M), name,
                " is a group-major cache [G, F, 128]: this operator takes the column-major [F, M] only");
    if (t.is_contiguous() && t.numel() == F * M) return M;
    TORCH_CHECK(t.dim() >= 2 && t.size(-2) == F && t.size(-1) == M && t.numel() == F * M, name, " must be [F, M]");
    TORCH_CHECK(t.stride(-1) == 1, name, ": the M elements of a column must be contiguous");
    return t.stride(-2);
}
void check_pitch(int64_t ldc, int64_t M, const char *name) {
    TORCH_CHECK(ldc >= M && ldc % 8 == 0, name, ": the column pitch (", ldc, " elements) must be at least M = ", M,
                " and a multiple of 8: a contiguous [F, M] cache with M % 8 != 0 is not supported, pass the [:, :M] view of a [F, ceil8(M)] buffer");
}
bool whole_groups(int64_t M, int64_t ldc) { return M % 128 == 0 && ldc == M; }
int64_t groups_of(int64_t M) { return (M + 127) / 128; }

// Batches (B > 1 sequences in one launch): a [B, M, K], c [B, M, F], the cache [B, F, M] (or the [..., :M] view of [B, F, ldc], any batch
// stride the C entry accepts), indices [B, G, F], counts [B, G].  2-D operands and B == 1 take exactly the entries they always took.
// Group-major cache (the operators added here, never the reference-schema ones): a cache of one dimension more than a -- [G, F, 128] for
// a [M, K], [B, G, F, 128] for a [B, M, K], G = ceil(M / 128) -- with each [G, F, 128] block contiguous; the batch stride is the tensor's.
// (A shape that is also a column-major one, [1, F, 128] for M = 128, holds the same elements either way and stays column-major.)
struct Mm1Shape {
    int64_t B, M, K, F, ldc, cache_bs;
    bool gm = false;
    bool batched() const { return B > 1; }
};
// (bias: null for the gated operator, which checks its two optional vectors itself)
Mm1Shape mm1_shape(const at::Tensor &a, const at::Tensor &b, const at::Tensor &c, const at::Tensor *bias, const at::Tensor &cache,
                   const at::Tensor &indices, const at::Tensor &counts, bool allow_gm = false) {
    TORCH_CHECK((a.dim() == 2 || a.dim() == 3) && b.dim() == 2 && c.dim() == a.dim(), "a and c must both be 2D ([M, .]) or 3D ([B, M, .]), b 2D");
    Mm1Shape s;
    s.B = a.dim() == 3 ? a.size(0) : 1;
    s.M = a.size(-2), s.K = a.size(-1), s.F = b.size(0);
    TORCH_CHECK(s.B >= 1, "the batch size must be at least 1");
    TORCH_CHECK(b.size(1) == s.K, "a and b must share the K dimension");
    TORCH_CHECK(c.size(-2) == s.M && c.size(-1) == s.F && c.numel() == s.B * s.M * s.F, "c must be [M, F] ([B, M, F] with the batch size of a)");
    if (bias) TORCH_CHECK(bias->numel() == s.F, "bias must have F entries");
    const int64_t G = groups_of(s.M);
    s.gm = allow_gm && cache.dim() == a.dim() + 1 &&
           !(cache.size(-2) == s.F && cache.size(-1) == s.M && cache.numel() == s.F * s.M && cache.is_contiguous());
    if (s.gm) {
        TORCH_CHECK(cache.size(-1) == 128 && cache.size(-2) == s.F && cache.size(-3) == G && (a.dim() == 2 || cache.size(0) == s.B),
                    "a group-major pa_cache must be [G, F, 128] ([B, G, F, 128] with the batch size of a), G = ceil(M / 128) = ", G, ", F = ", s.F,
                    " (got ", cache.sizes(), ")");
        TORCH_CHECK(cache.stride(-1) == 1 && cache.stride(-2) == 128 && (G == 1 || cache.stride(-3) == s.F * 128),
                    "a group-major pa_cache: each [G, F, 128] block must be contiguous");
        TORCH_CHECK(G * s.F * 128 < (1ll << 31), "a group-major pa_cache: G * F * 128 too large for 32-bit offsets");
        s.ldc = 128, s.cache_bs = a.dim() == 3 && s.B > 1 ? cache.stride(0) : G * s.F * 128;
        TORCH_CHECK(s.cache_bs >= G * s.F * 128 && s.cache_bs % 8 == 0, "a group-major pa_cache: the batch stride (", s.cache_bs,
                    " elements) must be at least G * F * 128 = ", G * s.F * 128, " and a multiple of 8");
    } else if (!s.batched()) {
        s.ldc = cache_pitch(cache, s.F, s.M, "pa_cache_colmajor");
        s.cache_bs = s.F * s.ldc;
    } else {
        TORCH_CHECK(cache.dim() == 3 && cache.size(0) == s.B && cache.size(1) == s.F && cache.size(2) == s.M,
                    "pa_cache_colmajor must be [B, F, M] with the batch size of a (B = ", s.B, ")");
        TORCH_CHECK(cache.stride(2) == 1, "pa_cache_colmajor: the M elements of a column must be contiguous");
        s.ldc = cache.stride(1), s.cache_bs = cache.stride(0);
        TORCH_CHECK(s.cache_bs >= s.F * s.ldc && s.cache_bs % 8 == 0, "pa_cache_colmajor: the batch stride (", s.cache_bs,
                    " elements) must be at least F * ldc = ", s.F * s.ldc, " and a multiple of 8");
    }
    if (!s.gm) check_pitch(s.ldc, s.M, "pa_cache_colmajor");
    TORCH_CHECK(indices.numel() == s.B * G * s.F && counts.numel() == s.B * G,
                "indices must be [ceil(M/128), F], counts [ceil(M/128)] ([B, ceil(M/128), F] and [B, ceil(M/128)] with the batch size of a)");
    TORCH_CHECK(s.B * G <= 65535, "B * ceil(M/128) groups must not exceed 65535 (got ", s.B * G, ")");
    return s;
}

Mm1Shape mm1_shape(const at::Tensor &a, const at::Tensor &b, const at::Tensor &c, const at::Tensor &bias, const at::Tensor &cache,
                   const at::Tensor &indices, const at::Tensor &counts) {
    return mm1_shape(a, b, c, &bias, cache, indices, counts);
}

// activation by name -> CHIPMUNK_ACT_*; who: the operator's name for the message
static int act_code(const char *who, const std::string &act) {
    int code = -1;
    if (act == "gelu_tanh") code = CHIPMUNK_ACT_GELU_TANH;
    else if (act == "silu") code = CHIPMUNK_ACT_SILU;
    else if (act == "gelu") code = CHIPMUNK_ACT_GELU_ERF;
    TORCH_CHECK(code >= 0, who, ": unknown activation '", act, "' (one of gelu_tanh, silu, gelu)");
    return code;
}
// an optional bias vector (bf16, F entries; name: the argument's, for the message): its pointer, null when it is not given
static const void *optional_bias(const c10::optional<at::Tensor> &bias, const char *name, int64_t F) {
    if (!bias.has_value()) return nullptr;
    const at::Tensor &t = *bias;
    CHECK_DEV(t); CHECK_BF16(t); CHECK_CONTIG(t);
    TORCH_CHECK(t.numel() == F, name, " must have F entries (got ", t.numel(), ", F = ", F, ")");
    return t.data_ptr();
}

// csp_mlp_mm1 (reference csrc/mlp/csp_mlp_mm1.cu:625-702) and csp_mlp_mm1_scatter: the same operands and checks in front of the
// operator's three C entries -- the batch, whole groups (the reference's contract), everything else
template <auto BATCHED, auto WHOLE, auto RAGGED>
static void mm1_impl(const char *who, at::Tensor a, at::Tensor b_colmajor, at::Tensor c, at::Tensor bias, at::Tensor pa_cache_colmajor,
                     at::Tensor indices, at::Tensor indices_counts) {
    CHECK_DEV(a); CHECK_DEV(b_colmajor); CHECK_DEV(c); CHECK_DEV(bias); CHECK_DEV(pa_cache_colmajor);
    CHECK_DEV(indices); CHECK_DEV(indices_counts);
    CHECK_BF16(a); CHECK_BF16(b_colmajor); CHECK_BF16(c); CHECK_BF16(bias); CHECK_BF16(pa_cache_colmajor);
    CHECK_I32(indices); CHECK_I32(indices_counts);
    CHECK_CONTIG(a); CHECK_CONTIG(b_colmajor); CHECK_CONTIG(c); CHECK_CONTIG(bias);
    CHECK_CONTIG(indices); CHECK_CONTIG(indices_counts);
    const Mm1Shape sh = mm1_shape(a, b_colmajor, c, bias, pa_cache_colmajor, indices, indices_counts);
    const int M = (int)sh.M, K = (int)sh.K, F = (int)sh.F, ldc = (int)sh.ldc;
    int *ip = indices.data_ptr<int>(), *cp = indices_counts.data_ptr<int>();
    c10::DeviceGuard guard(a.device());
    if (sh.batched())
        check(BATCHED(a.data_ptr(), b_colmajor.data_ptr(), c.data_ptr(), bias.data_ptr(), pa_cache_colmajor.data_ptr(), ip, cp, M, K, F, ldc,
                      (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else if (whole_groups(sh.M, sh.ldc))
        check(WHOLE(a.data_ptr(), b_colmajor.data_ptr(), c.data_ptr(), bias.data_ptr(), pa_cache_colmajor.data_ptr(), ip, cp, M, K, F,
                    cur_stream(a)), who);
    else
        check(RAGGED(a.data_ptr(), b_colmajor.data_ptr(), c.data_ptr(), bias.data_ptr(), pa_cache_colmajor.data_ptr(), ip, cp, M, K, F, ldc,
                     cur_stream(a)), who);
}
void csp_mlp_mm1(at::Tensor a, at::Tensor b_colmajor, at::Tensor c, at::Tensor bias, at::Tensor pa_cache_colmajor,
                 at::Tensor indices, at::Tensor indices_counts) {
    mm1_impl<chipmunk_csp_mlp_mm1_batched, chipmunk_csp_mlp_mm1, chipmunk_csp_mlp_mm1_ragged>(
        "csp_mlp_mm1", a, b_colmajor, c, bias, pa_cache_colmajor, indices, indices_counts);
}
// addition: GEMM1 + the scatter-add of its output into the activation cache, one kernel
void csp_mlp_mm1_scatter(at::Tensor a, at::Tensor b_colmajor, at::Tensor c, at::Tensor bias, at::Tensor pa_cache_colmajor,
                         at::Tensor indices, at::Tensor indices_counts) {
    mm1_impl<chipmunk_csp_mlp_mm1_scatter_batched, chipmunk_csp_mlp_mm1_scatter, chipmunk_csp_mlp_mm1_scatter_ragged>(
        "csp_mlp_mm1_scatter", a, b_colmajor, c, bias, pa_cache_colmajor, indices, indices_counts);
}

// addition: gated GEMM1 (SwiGLU / GEGLU), c = bf16(act(a b_gate^T + bias_gate) * (a b_up^T + bias_up) - cache); update_cache also applies
// the scatter-add of c to the cache.  2-D operands or the 3-D batch, the cache checks of csp_mlp_mm1.  bf16 operands (csp_mlp_mm1_glu, which
// refuses fp8 ones), or -- scales given -- a, b_gate, b_up float8_e4m3fn with the three reciprocal quantisation scales as one-element
// float32 device tensors (csp_mlp_mm1_glu_fp8).
static void mm1_glu_impl(const char *who, at::Tensor a, at::Tensor b_gate, at::Tensor b_up, at::Tensor c,
                         const c10::optional<at::Tensor> &bias_gate, const c10::optional<at::Tensor> &bias_up, at::Tensor pa_cache_colmajor,
                         at::Tensor indices, at::Tensor indices_counts, const at::Tensor *scale_a, const at::Tensor *scale_b_gate,
                         const at::Tensor *scale_b_up, const std::string &act, bool update_cache) {
    const bool fp8 = scale_a != nullptr;
    CHECK_DEV(a); CHECK_DEV(b_gate); CHECK_DEV(b_up); CHECK_DEV(c); CHECK_DEV(pa_cache_colmajor);
    CHECK_DEV(indices); CHECK_DEV(indices_counts);
    if (fp8) {
        TORCH_CHECK(a.scalar_type() == at::kFloat8_e4m3fn && b_gate.scalar_type() == at::kFloat8_e4m3fn && b_up.scalar_type() == at::kFloat8_e4m3fn,
                    who, ": a, b_gate and b_up must be float8_e4m3fn (OCP; gfx950 has no fnuz)");
    } else {
        CHECK_BF16(a); CHECK_BF16(b_gate); CHECK_BF16(b_up);
    }
    CHECK_BF16(c); CHECK_BF16(pa_cache_colmajor);
    CHECK_I32(indices); CHECK_I32(indices_counts);
    CHECK_CONTIG(a); CHECK_CONTIG(b_gate); CHECK_CONTIG(b_up); CHECK_CONTIG(c);
    CHECK_CONTIG(indices); CHECK_CONTIG(indices_counts);
    if (fp8)
        for (const at::Tensor *s : {scale_a, scale_b_gate, scale_b_up})
            TORCH_CHECK(s->is_cuda() && s->scalar_type() == at::kFloat && s->numel() == 1, who,
                        ": scale_a, scale_b_gate and scale_b_up must be one-element float32 tensors on the GPU");
    const Mm1Shape sh = mm1_shape(a, b_gate, c, nullptr, pa_cache_colmajor, indices, indices_counts, true);
    TORCH_CHECK(b_up.dim() == 2 && b_up.size(0) == sh.F && b_up.size(1) == sh.K, "b_up must have the shape of b_gate ([F, K])");
    const void *bg = optional_bias(bias_gate, "bias_gate", sh.F), *bu = optional_bias(bias_up, "bias_up", sh.F);
    const int code = act_code(who, act);
    c10::DeviceGuard guard(a.device());
    int *ip = indices.data_ptr<int>(), *cp = indices_counts.data_ptr<int>();
    const int M = (int)sh.M, K = (int)sh.K, F = (int)sh.F, ldc = (int)sh.ldc, upd = update_cache ? 1 : 0;
    if (fp8 && sh.gm)
        check(chipmunk_csp_mlp_mm1_glu_fp8_gm(a.data_ptr(), b_gate.data_ptr(), b_up.data_ptr(), c.data_ptr(), bg, bu, pa_cache_colmajor.data_ptr(),
                                              ip, cp, scale_a->data_ptr<float>(), scale_b_gate->data_ptr<float>(),
                                              scale_b_up->data_ptr<float>(), M, K, F, code, upd, (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else if (sh.gm)
        check(chipmunk_csp_mlp_mm1_glu_gm(a.data_ptr(), b_gate.data_ptr(), b_up.data_ptr(), c.data_ptr(), bg, bu, pa_cache_colmajor.data_ptr(),
                                          ip, cp, M, K, F, code, upd, (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else if (fp8 && sh.batched())
        check(chipmunk_csp_mlp_mm1_glu_fp8_batched(a.data_ptr(), b_gate.data_ptr(), b_up.data_ptr(), c.data_ptr(), bg, bu,
                                                   pa_cache_colmajor.data_ptr(), ip, cp, scale_a->data_ptr<float>(),
                                                   scale_b_gate->data_ptr<float>(), scale_b_up->data_ptr<float>(), M, K, F, ldc, code, upd,
                                                   (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else if (fp8)
        check(chipmunk_csp_mlp_mm1_glu_fp8(a.data_ptr(), b_gate.data_ptr(), b_up.data_ptr(), c.data_ptr(), bg, bu, pa_cache_colmajor.data_ptr(),
                                           ip, cp, scale_a->data_ptr<float>(), scale_b_gate->data_ptr<float>(),
                                           scale_b_up->data_ptr<float>(), M, K, F, ldc, code, upd, cur_stream(a)), who);
    else if (sh.batched())
        check(chipmunk_csp_mlp_mm1_glu_batched(a.data_ptr(), b_gate.data_ptr(), b_up.data_ptr(), c.data_ptr(), bg, bu,
                                               pa_cache_colmajor.data_ptr(), ip, cp, M, K, F, ldc, code, upd, (int)sh.B, sh.cache_bs,
                                               cur_stream(a)), who);
    else
        check(chipmunk_csp_mlp_mm1_glu(a.data_ptr(), b_gate.data_ptr(), b_up.data_ptr(), c.data_ptr(), bg, bu, pa_cache_colmajor.data_ptr(), ip,
                                       cp, M, K, F, ldc, code, upd, cur_stream(a)), who);
}
void csp_mlp_mm1_glu(at::Tensor a, at::Tensor b_gate, at::Tensor b_up, at::Tensor c, const c10::optional<at::Tensor> &bias_gate,
                     const c10::optional<at::Tensor> &bias_up, at::Tensor pa_cache_colmajor, at::Tensor indices, at::Tensor indices_counts,
                     std::string act, bool update_cache) {
    mm1_glu_impl("csp_mlp_mm1_glu", a, b_gate, b_up, c, bias_gate, bias_up, pa_cache_colmajor, indices, indices_counts, nullptr, nullptr, nullptr,
                 act, update_cache);
}
void csp_mlp_mm1_glu_fp8(at::Tensor a, at::Tensor b_gate, at::Tensor b_up, at::Tensor c, const c10::optional<at::Tensor> &bias_gate,
                         const c10::optional<at::Tensor> &bias_up, at::Tensor pa_cache_colmajor, at::Tensor indices, at::Tensor indices_counts,
                         at::Tensor scale_a, at::Tensor scale_b_gate, at::Tensor scale_b_up, std::string act, bool update_cache) {
    mm1_glu_impl("csp_mlp_mm1_glu_fp8", a, b_gate, b_up, c, bias_gate, bias_up, pa_cache_colmajor, indices, indices_counts, &scale_a,
                 &scale_b_gate, &scale_b_up, act, update_cache);
}

// native counterpart of the reference's Triton csp_mlp_mm1_fp8 (src/chipmunk/triton/csp_mlp_mm1.py:143-164)
static void mm1_fp8_impl(at::Tensor a, at::Tensor b, at::Tensor c, at::Tensor bias, at::Tensor pa_cache_colmajor,
                         at::Tensor indices, at::Tensor indices_counts, at::Tensor scale_a, at::Tensor scale_b,
                         int update_cache) {
    CHECK_DEV(a); CHECK_DEV(b); CHECK_DEV(c); CHECK_DEV(bias); CHECK_DEV(pa_cache_colmajor);
    CHECK_DEV(indices); CHECK_DEV(indices_counts); CHECK_DEV(scale_a); CHECK_DEV(scale_b);
    TORCH_CHECK(a.scalar_type() == at::kFloat8_e4m3fn && b.scalar_type() == at::kFloat8_e4m3fn,
                "a and b must be float8_e4m3fn (OCP; gfx950 has no fnuz)");
    CHECK_BF16(c); CHECK_BF16(bias); CHECK_BF16(pa_cache_colmajor);
    CHECK_I32(indices); CHECK_I32(indices_counts);
    CHECK_CONTIG(a); CHECK_CONTIG(b); CHECK_CONTIG(c); CHECK_CONTIG(bias);
    CHECK_CONTIG(indices); CHECK_CONTIG(indices_counts);
    TORCH_CHECK(scale_a.scalar_type() == at::kFloat && scale_b.scalar_type() == at::kFloat && scale_a.numel() == 1 &&
                scale_b.numel() == 1, "scale_a and scale_b must be one-element float32 tensors");
    const Mm1Shape sh = mm1_shape(a, b, c, bias, pa_cache_colmajor, indices, indices_counts);
    const int64_t M = sh.M, K = sh.K, F = sh.F, ldc = sh.ldc;
    c10::DeviceGuard guard(a.device());
    if (sh.batched())
        check(chipmunk_csp_mlp_mm1_fp8_batched(a.data_ptr(), b.data_ptr(), c.data_ptr(), bias.data_ptr(), pa_cache_colmajor.data_ptr(),
                                               indices.data_ptr<int>(), indices_counts.data_ptr<int>(), scale_a.data_ptr<float>(),
                                               scale_b.data_ptr<float>(), (int)M, (int)K, (int)F, (int)ldc, update_cache, (int)sh.B,
                                               sh.cache_bs, cur_stream(a)),
              "csp_mlp_mm1_fp8");
    else if (whole_groups(M, ldc))
        check(chipmunk_csp_mlp_mm1_fp8(a.data_ptr(), b.data_ptr(), c.data_ptr(), bias.data_ptr(),
                                       pa_cache_colmajor.data_ptr(), indices.data_ptr<int>(),
                                       indices_counts.data_ptr<int>(), scale_a.data_ptr<float>(), scale_b.data_ptr<float>(),
                                       (int)M, (int)K, (int)F, update_cache, cur_stream(a)),
              "csp_mlp_mm1_fp8");
    else
        check(chipmunk_csp_mlp_mm1_fp8_ragged(a.data_ptr(), b.data_ptr(), c.data_ptr(), bias.data_ptr(),
                                              pa_cache_colmajor.data_ptr(), indices.data_ptr<int>(),
                                              indices_counts.data_ptr<int>(), scale_a.data_ptr<float>(), scale_b.data_ptr<float>(),
                                              (int)M, (int)K, (int)F, (int)ldc, update_cache, cur_stream(a)),
              "csp_mlp_mm1_fp8");
}

void csp_mlp_mm1_fp8(at::Tensor a, at::Tensor b, at::Tensor c, at::Tensor bias, at::Tensor pa_cache_colmajor,
                     at::Tensor indices, at::Tensor indices_counts, at::Tensor scale_a, at::Tensor scale_b,
                     bool update_cache) {
    mm1_fp8_impl(a, b, c, bias, pa_cache_colmajor, indices, indices_counts, scale_a, scale_b, update_cache ? 1 : 0);
}
// fp8 GEMM1 that applies the scatter-add of its own deltas to the cache (the fp8 counterpart of csp_mlp_mm1_scatter)
void csp_mlp_mm1_fp8_scatter(at::Tensor a, at::Tensor b, at::Tensor c, at::Tensor bias, at::Tensor pa_cache_colmajor,
                             at::Tensor indices, at::Tensor indices_counts, at::Tensor scale_a, at::Tensor scale_b) {
    mm1_fp8_impl(a, b, c, bias, pa_cache_colmajor, indices, indices_counts, scale_a, scale_b, 2);
}

// addition: the ungated GEMM1 with the activation by name and an optional bias, c = bf16(act(a b^T + bias) - cache); bf16 operands, or
// (scale_a / scale_b given) e4m3 a / b in the arithmetic of csp_mlp_mm1_fp8.  2-D operands or the 3-D batch, always the ragged contract.
// update_cache: the C entries' (bf16 0 / 1; fp8 0 / 1 / 2).  rs: scale_a is a vector over the token rows ([M]; [B, M] for a batch), scale_b one
// over the fc1 columns ([F]) -- csp_mlp_mm1_fp8_act_rs.
static void mm1_act_impl(const char *who, at::Tensor a, at::Tensor b, at::Tensor c, const c10::optional<at::Tensor> &bias,
                         at::Tensor pa_cache_colmajor, at::Tensor indices, at::Tensor indices_counts, const at::Tensor *scale_a,
                         const at::Tensor *scale_b, const std::string &act, int update_cache, bool rs = false) {
    const bool fp8 = scale_a != nullptr;
    CHECK_DEV(a); CHECK_DEV(b); CHECK_DEV(c); CHECK_DEV(pa_cache_colmajor);
    CHECK_DEV(indices); CHECK_DEV(indices_counts);
    if (fp8) {
        TORCH_CHECK(a.scalar_type() == at::kFloat8_e4m3fn && b.scalar_type() == at::kFloat8_e4m3fn,
                    who, ": a and b must be float8_e4m3fn (OCP; gfx950 has no fnuz)");
        for (const at::Tensor *s : {scale_a, scale_b})
            TORCH_CHECK(s->is_cuda() && s->scalar_type() == at::kFloat && (rs || s->numel() == 1), who,
                        rs ? ": scale_a and scale_b must be float32 tensors on the GPU" : ": scale_a and scale_b must be one-element float32 tensors on the GPU");
        if (rs) {
            TORCH_CHECK(scale_a->device() == a.device() && scale_b->device() == a.device(), who, ": scale_a and scale_b must be on the device of a");
            TORCH_CHECK(scale_a->is_contiguous() && scale_b->is_contiguous(), who, ": scale_a and scale_b must be contiguous");
            TORCH_CHECK((a.dim() == 2 && scale_a->dim() == 1 && scale_a->size(0) == a.size(0)) ||
                            (a.dim() == 3 && scale_a->dim() == 2 && scale_a->size(0) == a.size(0) && scale_a->size(1) == a.size(1)),
                        who, ": scale_a must be [M], one reciprocal scale per row of a ([B, M] for a batched a)");
            TORCH_CHECK(scale_b->dim() == 1 && b.dim() == 2 && scale_b->size(0) == b.size(0), who,
                        ": scale_b must be [F], one reciprocal scale per row of b");
        }
    } else {
        CHECK_BF16(a); CHECK_BF16(b);
    }
    CHECK_BF16(c); CHECK_BF16(pa_cache_colmajor);
    CHECK_I32(indices); CHECK_I32(indices_counts);
    CHECK_CONTIG(a); CHECK_CONTIG(b); CHECK_CONTIG(c);
    CHECK_CONTIG(indices); CHECK_CONTIG(indices_counts);
    const Mm1Shape sh = mm1_shape(a, b, c, nullptr, pa_cache_colmajor, indices, indices_counts, true);
    const void *bp = optional_bias(bias, "bias", sh.F);
    const int code = act_code(who, act);
    c10::DeviceGuard guard(a.device());
    int *ip = indices.data_ptr<int>(), *cp = indices_counts.data_ptr<int>();
    const int M = (int)sh.M, K = (int)sh.K, F = (int)sh.F, ldc = (int)sh.ldc;
    if (rs && sh.gm)
        check(chipmunk_csp_mlp_mm1_fp8_act_rs_gm(a.data_ptr(), b.data_ptr(), c.data_ptr(), bp, pa_cache_colmajor.data_ptr(), ip, cp,
                                                 scale_a->data_ptr<float>(), scale_b->data_ptr<float>(), M, K, F, code, update_cache,
                                                 (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else if (fp8 && sh.gm)
        check(chipmunk_csp_mlp_mm1_fp8_act_gm(a.data_ptr(), b.data_ptr(), c.data_ptr(), bp, pa_cache_colmajor.data_ptr(), ip, cp,
                                              scale_a->data_ptr<float>(), scale_b->data_ptr<float>(), M, K, F, code, update_cache,
                                              (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else if (sh.gm)
        check(chipmunk_csp_mlp_mm1_act_gm(a.data_ptr(), b.data_ptr(), c.data_ptr(), bp, pa_cache_colmajor.data_ptr(), ip, cp, M, K, F, code,
                                          update_cache, (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else if (rs && sh.batched())
        check(chipmunk_csp_mlp_mm1_fp8_act_rs_batched(a.data_ptr(), b.data_ptr(), c.data_ptr(), bp, pa_cache_colmajor.data_ptr(), ip, cp,
                                                      scale_a->data_ptr<float>(), scale_b->data_ptr<float>(), M, K, F, ldc, code,
                                                      update_cache, (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else if (rs)
        check(chipmunk_csp_mlp_mm1_fp8_act_rs(a.data_ptr(), b.data_ptr(), c.data_ptr(), bp, pa_cache_colmajor.data_ptr(), ip, cp,
                                              scale_a->data_ptr<float>(), scale_b->data_ptr<float>(), M, K, F, ldc, code, update_cache,
                                              cur_stream(a)), who);
    else if (fp8 && sh.batched())
        check(chipmunk_csp_mlp_mm1_fp8_act_batched(a.data_ptr(), b.data_ptr(), c.data_ptr(), bp, pa_cache_colmajor.data_ptr(), ip, cp,
                                                   scale_a->data_ptr<float>(), scale_b->data_ptr<float>(), M, K, F, ldc, code,
                                                   update_cache, (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else if (fp8)
        check(chipmunk_csp_mlp_mm1_fp8_act(a.data_ptr(), b.data_ptr(), c.data_ptr(), bp, pa_cache_colmajor.data_ptr(), ip, cp,
                                           scale_a->data_ptr<float>(), scale_b->data_ptr<float>(), M, K, F, ldc, code, update_cache,
                                           cur_stream(a)), who);
    else if (sh.batched())
        check(chipmunk_csp_mlp_mm1_act_batched(a.data_ptr(), b.data_ptr(), c.data_ptr(), bp, pa_cache_colmajor.data_ptr(), ip, cp, M, K, F,
                                               ldc, code, update_cache, (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else
        check(chipmunk_csp_mlp_mm1_act(a.data_ptr(), b.data_ptr(), c.data_ptr(), bp, pa_cache_colmajor.data_ptr(), ip, cp, M, K, F, ldc,
                                       code, update_cache, cur_stream(a)), who);
}
void csp_mlp_mm1_act(at::Tensor a, at::Tensor b, at::Tensor c, const c10::optional<at::Tensor> &bias, at::Tensor pa_cache,
                     at::Tensor indices, at::Tensor counts, std::string act, bool update_cache) {
    mm1_act_impl("csp_mlp_mm1_act", a, b, c, bias, pa_cache, indices, counts, nullptr, nullptr, act, update_cache ? 1 : 0);
}
void csp_mlp_mm1_fp8_act(at::Tensor a, at::Tensor b, at::Tensor c, const c10::optional<at::Tensor> &bias, at::Tensor pa_cache,
                         at::Tensor indices, at::Tensor counts, at::Tensor scale_a, at::Tensor scale_b, std::string act,
                         int64_t update_cache) {
    TORCH_CHECK(update_cache >= 0 && update_cache <= 2, "csp_mlp_mm1_fp8_act: update_cache must be 0, 1 or 2 (got ", update_cache, ")");
    mm1_act_impl("csp_mlp_mm1_fp8_act", a, b, c, bias, pa_cache, indices, counts, &scale_a, &scale_b, act, (int)update_cache);
}
// addition: csp_mlp_mm1_fp8_act with one reciprocal scale per token row (scale_a [M] / [B, M]) and one per fc1 column (scale_b [F], read at
// the gathered column): t = bf16(act((a b^T * scale_a[m]) * scale_b[i] + bias[i])), c = bf16(t - cache)
void csp_mlp_mm1_fp8_act_rs(at::Tensor a, at::Tensor b, at::Tensor c, const c10::optional<at::Tensor> &bias, at::Tensor pa_cache,
                            at::Tensor indices, at::Tensor counts, at::Tensor scale_a, at::Tensor scale_b, std::string act,
                            int64_t update_cache) {
    TORCH_CHECK(update_cache >= 0 && update_cache <= 2, "csp_mlp_mm1_fp8_act_rs: update_cache must be 0, 1 or 2 (got ", update_cache, ")");
    mm1_act_impl("csp_mlp_mm1_fp8_act_rs", a, b, c, bias, pa_cache, indices, counts, &scale_a, &scale_b, act, (int)update_cache, true);
}

// addition: csp_mlp_mm1_act over an e4m3 weight with bf16 activations (weight-only fp8, chipmunk_csp_mlp_mm1_w8): scale_b is the weight's
// float32 reciprocal scale -- one element, or [F] with one per row of b --, c = bf16(act((a f(b)^T) * scale_b + bias) - cache)
void csp_mlp_mm1_w8(at::Tensor a, at::Tensor b, at::Tensor scale_b, at::Tensor c, const c10::optional<at::Tensor> &bias, at::Tensor pa_cache,
                    at::Tensor indices, at::Tensor counts, std::string act, bool update_cache) {
    const char *who = "csp_mlp_mm1_w8";
    CHECK_DEV(a); CHECK_DEV(b); CHECK_DEV(scale_b); CHECK_DEV(c); CHECK_DEV(pa_cache); CHECK_DEV(indices); CHECK_DEV(counts);
    CHECK_BF16(a);
    TORCH_CHECK(b.scalar_type() == at::kFloat8_e4m3fn, who, ": b must be float8_e4m3fn (OCP; gfx950 has no fnuz)");
    CHECK_BF16(c); CHECK_BF16(pa_cache);
    CHECK_I32(indices); CHECK_I32(counts);
    CHECK_CONTIG(a); CHECK_CONTIG(b); CHECK_CONTIG(c); CHECK_CONTIG(indices); CHECK_CONTIG(counts);
    const Mm1Shape sh = mm1_shape(a, b, c, nullptr, pa_cache, indices, counts, true);
    TORCH_CHECK(scale_b.scalar_type() == at::kFloat && scale_b.is_contiguous() && scale_b.device() == a.device() &&
                    (scale_b.numel() == 1 || (scale_b.dim() == 1 && scale_b.size(0) == sh.F)),
                who, ": scale_b must be a contiguous float32 tensor on the device of a with one element, or [F] with one reciprocal scale per row of b");
    const void *bp = optional_bias(bias, "bias", sh.F);
    const int code = act_code(who, act);
    c10::DeviceGuard guard(a.device());
    int *ip = indices.data_ptr<int>(), *cp = counts.data_ptr<int>();
    const int M = (int)sh.M, K = (int)sh.K, F = (int)sh.F, ldc = (int)sh.ldc, sn = (int)scale_b.numel(), upd = update_cache ? 1 : 0;
    const float *sp = scale_b.data_ptr<float>();
    if (sh.gm)
        check(chipmunk_csp_mlp_mm1_w8_gm(a.data_ptr(), b.data_ptr(), sp, sn, c.data_ptr(), bp, pa_cache.data_ptr(), ip, cp, M, K, F, code, upd,
                                         (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else if (sh.batched())
        check(chipmunk_csp_mlp_mm1_w8_batched(a.data_ptr(), b.data_ptr(), sp, sn, c.data_ptr(), bp, pa_cache.data_ptr(), ip, cp, M, K, F, ldc,
                                              code, upd, (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else
        check(chipmunk_csp_mlp_mm1_w8(a.data_ptr(), b.data_ptr(), sp, sn, c.data_ptr(), bp, pa_cache.data_ptr(), ip, cp, M, K, F, ldc, code,
                                      upd, cur_stream(a)), who);
}

// addition: csp_mlp_mm1_glu over e4m3 gate / up weights with bf16 activations (gated weight-only fp8, chipmunk_csp_mlp_mm1_glu_w8): scale_gate /
// scale_up are the weights' float32 reciprocal scales -- one element, or [F] with one per row --,
// c = bf16(fma(act((a f(b_gate)^T) * scale_gate + bias_gate), (a f(b_up)^T) * scale_up + bias_up, -cache))
void csp_mlp_mm1_glu_w8(at::Tensor a, at::Tensor b_gate, at::Tensor b_up, at::Tensor scale_gate, at::Tensor scale_up, at::Tensor c,
                        const c10::optional<at::Tensor> &bias_gate, const c10::optional<at::Tensor> &bias_up, at::Tensor pa_cache,
                        at::Tensor indices, at::Tensor counts, std::string act, bool update_cache) {
    const char *who = "csp_mlp_mm1_glu_w8";
    CHECK_DEV(a); CHECK_DEV(b_gate); CHECK_DEV(b_up); CHECK_DEV(scale_gate); CHECK_DEV(scale_up); CHECK_DEV(c); CHECK_DEV(pa_cache);
    CHECK_DEV(indices); CHECK_DEV(counts);
    CHECK_BF16(a);
    TORCH_CHECK(b_gate.scalar_type() == at::kFloat8_e4m3fn && b_up.scalar_type() == at::kFloat8_e4m3fn, who,
                ": b_gate and b_up must be float8_e4m3fn (OCP; gfx950 has no fnuz)");
    CHECK_BF16(c); CHECK_BF16(pa_cache);
    CHECK_I32(indices); CHECK_I32(counts);
    CHECK_CONTIG(a); CHECK_CONTIG(b_gate); CHECK_CONTIG(b_up); CHECK_CONTIG(c); CHECK_CONTIG(indices); CHECK_CONTIG(counts);
    const Mm1Shape sh = mm1_shape(a, b_gate, c, nullptr, pa_cache, indices, counts, true);
    TORCH_CHECK(b_up.dim() == 2 && b_up.size(0) == sh.F && b_up.size(1) == sh.K, "b_up must have the shape of b_gate ([F, K])");
    for (const at::Tensor *s : {&scale_gate, &scale_up})
        TORCH_CHECK(s->scalar_type() == at::kFloat && s->is_contiguous() && s->device() == a.device() &&
                        (s->numel() == 1 || (s->dim() == 1 && s->size(0) == sh.F)),
                    who, ": scale_gate and scale_up must be contiguous float32 tensors on the device of a with one element, or [F] with one "
                         "reciprocal scale per weight row");
    const void *bg = optional_bias(bias_gate, "bias_gate", sh.F), *bu = optional_bias(bias_up, "bias_up", sh.F);
    const int code = act_code(who, act);
    c10::DeviceGuard guard(a.device());
    int *ip = indices.data_ptr<int>(), *cp = counts.data_ptr<int>();
    const int M = (int)sh.M, K = (int)sh.K, F = (int)sh.F, ldc = (int)sh.ldc, upd = update_cache ? 1 : 0;
    const int gn = (int)scale_gate.numel(), un = (int)scale_up.numel();
    const float *gp = scale_gate.data_ptr<float>(), *up = scale_up.data_ptr<float>();
    if (sh.gm)
        check(chipmunk_csp_mlp_mm1_glu_w8_gm(a.data_ptr(), b_gate.data_ptr(), b_up.data_ptr(), gp, gn, up, un, c.data_ptr(), bg, bu,
                                             pa_cache.data_ptr(), ip, cp, M, K, F, code, upd, (int)sh.B, sh.cache_bs, cur_stream(a)), who);
    else if (sh.batched())
        check(chipmunk_csp_mlp_mm1_glu_w8_batched(a.data_ptr(), b_gate.data_ptr(), b_up.data_ptr(), gp, gn, up, un, c.data_ptr(), bg, bu,
                                                  pa_cache.data_ptr(), ip, cp, M, K, F, ldc, code, upd, (int)sh.B, sh.cache_bs, cur_stream(a)),
              who);
    else
        check(chipmunk_csp_mlp_mm1_glu_w8(a.data_ptr(), b_gate.data_ptr(), b_up.data_ptr(), gp, gn, up, un, c.data_ptr(), bg, bu,
                                          pa_cache.data_ptr(), ip, cp, M, K, F, ldc, code, upd, cur_stream(a)), who);
}

// addition: the weight-only fp8 linear layer for few rows (chipmunk_w8_linear): y = bf16(bf16((x f(w)^T) * scale_b) + bias), x [M, K] bf16 with
// contiguous rows (any row pitch), w [F, K] e4m3, scale_b float32 with one element or [F], y [M, F] bf16 (any row pitch), written in place
void w8_linear(at::Tensor x, at::Tensor w, at::Tensor scale_b, const c10::optional<at::Tensor> &bias, at::Tensor y) {
    const char *who = "w8_linear";
    CHECK_DEV(x); CHECK_DEV(w); CHECK_DEV(scale_b); CHECK_DEV(y);
    CHECK_BF16(x); CHECK_BF16(y);
    TORCH_CHECK(w.scalar_type() == at::kFloat8_e4m3fn, who, ": w must be float8_e4m3fn (OCP; gfx950 has no fnuz)");
    CHECK_CONTIG(w);
    TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && y.dim() == 2 && x.size(1) == w.size(1) && y.size(0) == x.size(0) && y.size(1) == w.size(0),
                who, ": x must be [M, K], w [F, K] and y [M, F]");
    TORCH_CHECK(x.size(0) >= 1 && x.stride(1) == 1 && y.stride(1) == 1, who, ": x and y need at least one row and contiguous rows");
    TORCH_CHECK(w.device() == x.device() && y.device() == x.device(), who, ": w and y must be on the device of x");
    const int64_t M = x.size(0), K = x.size(1), F = w.size(0);
    TORCH_CHECK(M <= CHIPMUNK_W8_LINEAR_MAX_M && K < (int64_t(1) << 31) && F < (int64_t(1) << 31), who, ": M, K or F too large");
    TORCH_CHECK(scale_b.scalar_type() == at::kFloat && scale_b.is_contiguous() && scale_b.device() == x.device() &&
                    (scale_b.numel() == 1 || (scale_b.dim() == 1 && scale_b.size(0) == F)),
                who, ": scale_b must be a contiguous float32 tensor on the device of x with one element, or [F] with one reciprocal scale per row of w");
    const void *bp = optional_bias(bias, "bias", F);
    c10::DeviceGuard guard(x.device());
    const int64_t ldx = M > 1 ? x.stride(0) : K, ldy = M > 1 ? y.stride(0) : F;
    check(chipmunk_w8_linear(x.data_ptr(), ldx, w.data_ptr(), scale_b.data_ptr<float>(), (int)scale_b.numel(), bp, y.data_ptr(), ldy, (int)M,
                             (int)K, (int)F, cur_stream(x)), who);
}

int64_t check_scatter_args(const at::Tensor &packed, const at::Tensor &unpacked, const at::Tensor &inds,
                           const at::Tensor &counts, int64_t *cache_bs) {   // returns the cache pitch; *cache_bs: the cache's batch stride
    // reference csrc/indexed_io/scatter_add.cu:111-142 (B is hard-wired to 1, :58-59,138)
    CHECK_DEV(packed); CHECK_DEV(unpacked); CHECK_DEV(inds); CHECK_DEV(counts);
    CHECK_CONTIG(packed); CHECK_CONTIG(inds); CHECK_CONTIG(counts);
    TORCH_CHECK(packed.dim() == 3, "packed must be a 3D tensor");
    TORCH_CHECK(unpacked.dim() == 3, "unpacked_colmajor must be a 3D tensor");
    TORCH_CHECK(inds.dim() == 3, "sp_inds must be a 3D tensor");
    TORCH_CHECK(counts.dim() == 2, "sp_counts must be a 2D tensor");
    CHECK_BF16(packed); CHECK_BF16(unpacked);
    CHECK_I32(inds); CHECK_I32(counts);
    // (the reference hard-wires a batch of 1; here the leading dimension is the number of sequences of one launch)
    const int64_t B = packed.size(0), M = packed.size(1), F = packed.size(2);
    TORCH_CHECK(B >= 1, "batch size must be at least 1");
    TORCH_CHECK(unpacked.size(0) == B && inds.size(0) == B && counts.size(0) == B,
                "packed, unpacked_colmajor, sp_inds and sp_counts must share the batch size (packed has B = ", B, ")");
    TORCH_CHECK(unpacked.size(1) == F && unpacked.size(2) == M, "unpacked_colmajor must be [B, F, M]");
    TORCH_CHECK(inds.size(1) == groups_of(M) && inds.size(2) == F, "sp_inds must be [B, ceil(M/128), F]");
    TORCH_CHECK(counts.size(1) == groups_of(M), "sp_counts must be [B, ceil(M/128)]");
    TORCH_CHECK(B * groups_of(M) <= 65535, "B * ceil(M/128) groups must not exceed 65535 (got ", B * groups_of(M), ")");
    int64_t ldc;
    if (B == 1) {
        ldc = cache_pitch(unpacked, F, M, "unpacked_colmajor");
        *cache_bs = F * ldc;
    } else {
        TORCH_CHECK(unpacked.stride(2) == 1, "unpacked_colmajor: the M elements of a column must be contiguous");
        ldc = unpacked.stride(1), *cache_bs = unpacked.stride(0);
        TORCH_CHECK(*cache_bs >= F * ldc && *cache_bs % 8 == 0, "unpacked_colmajor: the batch stride (", *cache_bs,
                    " elements) must be at least F * ldc = ", F * ldc, " and a multiple of 8");
    }
    check_pitch(ldc, M, "unpacked_colmajor");
    return ldc;
}

// reference csrc/indexed_io/scatter_add.cu:102-181
void csp_scatter_add(at::Tensor packed, at::Tensor unpacked_colmajor, at::Tensor sp_inds, at::Tensor sp_counts,
                     int64_t num_sms) {
    int64_t cache_bs = 0;
    const int64_t ldc = check_scatter_args(packed, unpacked_colmajor, sp_inds, sp_counts, &cache_bs);
    c10::DeviceGuard guard(packed.device());
    if (packed.size(0) > 1)
        check(chipmunk_csp_scatter_add_batched(packed.data_ptr(), unpacked_colmajor.data_ptr(), sp_inds.data_ptr<int>(),
                                               sp_counts.data_ptr<int>(), (int)packed.size(1), (int)packed.size(2), (int)ldc,
                                               (int)packed.size(0), cache_bs, cur_stream(packed)),
              "csp_scatter_add");
    else if (whole_groups(packed.size(1), ldc))
        check(chipmunk_csp_scatter_add(packed.data_ptr(), unpacked_colmajor.data_ptr(), sp_inds.data_ptr<int>(),
                                       sp_counts.data_ptr<int>(), (int)packed.size(1), (int)packed.size(2), (int)num_sms,
                                       cur_stream(packed)),
              "csp_scatter_add");
    else
        check(chipmunk_csp_scatter_add_ragged(packed.data_ptr(), unpacked_colmajor.data_ptr(), sp_inds.data_ptr<int>(),
                                              sp_counts.data_ptr<int>(), (int)packed.size(1), (int)packed.size(2), (int)ldc,
                                              cur_stream(packed)),
              "csp_scatter_add");
}

// addition: csp_scatter_add on the group-major cache.  packed [B, M, F], unpacked_groups [B, G, F, 128] (each [G, F, 128] block contiguous,
// any batch stride the C entry accepts), sp_inds [B, G, F], sp_counts [B, G]
void csp_scatter_add_gm(at::Tensor packed, at::Tensor unpacked_groups, at::Tensor sp_inds, at::Tensor sp_counts) {
    CHECK_DEV(packed); CHECK_DEV(unpacked_groups); CHECK_DEV(sp_inds); CHECK_DEV(sp_counts);
    CHECK_CONTIG(packed); CHECK_CONTIG(sp_inds); CHECK_CONTIG(sp_counts);
    CHECK_BF16(packed); CHECK_BF16(unpacked_groups);
    CHECK_I32(sp_inds); CHECK_I32(sp_counts);
    TORCH_CHECK(packed.dim() == 3 && unpacked_groups.dim() == 4 && sp_inds.dim() == 3 && sp_counts.dim() == 2,
                "csp_scatter_add_gm: packed [B, M, F], unpacked_groups [B, G, F, 128], sp_inds [B, G, F], sp_counts [B, G]");
    const int64_t B = packed.size(0), M = packed.size(1), F = packed.size(2), G = groups_of(M);
    TORCH_CHECK(B >= 1 && M >= 1, "csp_scatter_add_gm: batch size and M must be at least 1");
    TORCH_CHECK(unpacked_groups.size(0) == B && unpacked_groups.size(1) == G && unpacked_groups.size(2) == F && unpacked_groups.size(3) == 128,
                "csp_scatter_add_gm: unpacked_groups must be [B, G, F, 128] with G = ceil(M / 128) = ", G, ", F = ", F, " (got ",
                unpacked_groups.sizes(), ")");
    TORCH_CHECK(unpacked_groups.stride(3) == 1 && unpacked_groups.stride(2) == 128 && (G == 1 || unpacked_groups.stride(1) == F * 128),
                "csp_scatter_add_gm: each [G, F, 128] block of unpacked_groups must be contiguous");
    TORCH_CHECK(sp_inds.size(0) == B && sp_inds.size(1) == G && sp_inds.size(2) == F && sp_counts.size(0) == B && sp_counts.size(1) == G,
                "csp_scatter_add_gm: sp_inds must be [B, ceil(M/128), F], sp_counts [B, ceil(M/128)]");
    const int64_t cache_bs = B > 1 ? unpacked_groups.stride(0) : G * F * 128;
    c10::DeviceGuard guard(packed.device());
    check(chipmunk_csp_scatter_add_gm(packed.data_ptr(), unpacked_groups.data_ptr(), sp_inds.data_ptr<int>(), sp_counts.data_ptr<int>(), (int)M,
                                      (int)F, (int)B, cache_bs, cur_stream(packed)),
          "csp_scatter_add_gm");
}

// reference csrc/mlp/csp_mlp_mm2_and_scatter_add.cu:96-259.  `matmul_kernel` is the reference's Triton CUfunction
// smuggled as an int (:170); the GEMM is native here so the value is accepted and ignored.
void csp_mlp_mm2_and_scatter_add(at::Tensor packed, at::Tensor unpacked_colmajor, at::Tensor sp_inds,
                                 at::Tensor sp_counts, at::Tensor mma_a, at::Tensor mma_b, at::Tensor mma_c,
                                 int64_t num_sms_scatter_add, int64_t matmul_kernel) {
    (void)matmul_kernel;
    int64_t cache_bs = 0;
    const int64_t ldc = check_scatter_args(packed, unpacked_colmajor, sp_inds, sp_counts, &cache_bs);
    CHECK_DEV(mma_a); CHECK_DEV(mma_b); CHECK_DEV(mma_c);
    CHECK_BF16(mma_a); CHECK_BF16(mma_b); CHECK_BF16(mma_c);
    CHECK_CONTIG(mma_a); CHECK_CONTIG(mma_b); CHECK_CONTIG(mma_c);
    TORCH_CHECK(mma_a.dim() == 3 && mma_b.dim() == 3 && mma_c.dim() == 3, "mma_a, mma_b, mma_c must be 3D tensors");
    const int64_t B = packed.size(0), M = packed.size(1), F = packed.size(2), N2 = mma_b.size(2);
    TORCH_CHECK(mma_a.size(0) == B && mma_a.size(1) == M && mma_a.size(2) == F, "mma_a must be [B, M, F] with the batch size of packed (B = ", B, ")");
    TORCH_CHECK(mma_b.size(0) == 1 && mma_b.size(1) == F, "mma_b must be [1, F, N]");
    TORCH_CHECK(mma_c.size(0) == B && mma_c.size(1) == M && mma_c.size(2) == N2, "mma_c must be [B, M, N] with the batch size of packed (B = ", B, ")");
    c10::DeviceGuard guard(packed.device());
    if (B > 1)
        check(chipmunk_csp_mlp_mm2_and_scatter_add_batched(packed.data_ptr(), unpacked_colmajor.data_ptr(), sp_inds.data_ptr<int>(),
                                                           sp_counts.data_ptr<int>(), mma_a.data_ptr(), mma_b.data_ptr(), mma_c.data_ptr(),
                                                           (int)M, (int)F, (int)N2, (int)ldc, (int)B, cache_bs, cur_stream(packed)),
              "csp_mlp_mm2_and_scatter_add");
    else if (whole_groups(M, ldc))
        check(chipmunk_csp_mlp_mm2_and_scatter_add(packed.data_ptr(), unpacked_colmajor.data_ptr(),
                                                   sp_inds.data_ptr<int>(), sp_counts.data_ptr<int>(), mma_a.data_ptr(),
                                                   mma_b.data_ptr(), mma_c.data_ptr(), (int)M, (int)F, (int)N2,
                                                   (int)num_sms_scatter_add, cur_stream(packed)),
              "csp_mlp_mm2_and_scatter_add");
    else
        check(chipmunk_csp_mlp_mm2_and_scatter_add_ragged(packed.data_ptr(), unpacked_colmajor.data_ptr(),
                                                          sp_inds.data_ptr<int>(), sp_counts.data_ptr<int>(), mma_a.data_ptr(),
                                                          mma_b.data_ptr(), mma_c.data_ptr(), (int)M, (int)F, (int)N2, (int)ldc,
                                                          cur_stream(packed)),
              "csp_mlp_mm2_and_scatter_add");
}

// native counterpart of the reference's Triton csp_mlp_mm2 (src/chipmunk/triton/csp_mlp_mm2.py:104-129)
void csp_mlp_mm2(at::Tensor mma_a, at::Tensor mma_b, at::Tensor indices, at::Tensor counts, at::Tensor mma_c) {
    CHECK_DEV(mma_a); CHECK_DEV(mma_b); CHECK_DEV(mma_c); CHECK_DEV(indices); CHECK_DEV(counts);
    CHECK_BF16(mma_a); CHECK_BF16(mma_b); CHECK_BF16(mma_c);
    CHECK_I32(indices); CHECK_I32(counts);
    CHECK_CONTIG(mma_a); CHECK_CONTIG(mma_b); CHECK_CONTIG(mma_c); CHECK_CONTIG(indices); CHECK_CONTIG(counts);
    TORCH_CHECK((mma_a.dim() == 2 || mma_a.dim() == 3) && mma_b.dim() == 2 && mma_c.dim() == mma_a.dim(),
                "mma_a and mma_c must both be 2D ([M, .]) or 3D ([B, M, .]) tensors, mma_b 2D");
    const int64_t B = mma_a.dim() == 3 ? mma_a.size(0) : 1;
    const int64_t M = mma_a.size(-2), F = mma_a.size(-1), N2 = mma_b.size(1);
    TORCH_CHECK(B >= 1, "the batch size must be at least 1");
    TORCH_CHECK(mma_b.size(0) == F && mma_c.size(-2) == M && mma_c.size(-1) == N2 && mma_c.numel() == B * M * N2,
                "shape mismatch (mma_c must be [M, N2], or [B, M, N2] with the batch size of mma_a)");
    c10::DeviceGuard guard(mma_a.device());
    TORCH_CHECK(indices.numel() == B * groups_of(M) * F && counts.numel() == B * groups_of(M),
                "indices must be [ceil(M/128), F], counts [ceil(M/128)] ([B, ceil(M/128), F] and [B, ceil(M/128)] with the batch size of mma_a)");
    TORCH_CHECK(B * groups_of(M) <= 65535, "B * ceil(M/128) groups must not exceed 65535 (got ", B * groups_of(M), ")");
    if (B > 1) {
        check(chipmunk_csp_mlp_mm2_batched(mma_a.data_ptr(), mma_b.data_ptr(), mma_c.data_ptr(), indices.data_ptr<int>(),
                                           counts.data_ptr<int>(), (int)M, (int)F, (int)N2, (int)B, cur_stream(mma_a)),
              "csp_mlp_mm2");
        return;
    }
    check((M % 128 == 0 ? chipmunk_csp_mlp_mm2 : chipmunk_csp_mlp_mm2_ragged)(
              mma_a.data_ptr(), mma_b.data_ptr(), mma_c.data_ptr(), indices.data_ptr<int>(), counts.data_ptr<int>(), (int)M, (int)F,
              (int)N2, cur_stream(mma_a)),
          "csp_mlp_mm2");
}

// GEMM2 over e4m3 rows of fc2^T (weight-only fp8, chipmunk_csp_mlp_mm2_w8): csp_mlp_mm2 with mma_b float8_e4m3fn and its reciprocal scale
void csp_mlp_mm2_w8(at::Tensor mma_a, at::Tensor mma_b, at::Tensor scale_b, at::Tensor indices, at::Tensor counts, at::Tensor mma_c) {
    CHECK_DEV(mma_a); CHECK_DEV(mma_b); CHECK_DEV(mma_c); CHECK_DEV(indices); CHECK_DEV(counts);
    TORCH_CHECK(mma_b.scalar_type() == at::kFloat8_e4m3fn, "mma_b must be float8_e4m3fn (OCP; gfx950 has no fnuz)");
    TORCH_CHECK(scale_b.is_cuda() && scale_b.scalar_type() == at::kFloat && scale_b.numel() == 1,
                "scale_b must be a one-element float32 tensor on the GPU");
    CHECK_BF16(mma_a); CHECK_BF16(mma_c);
    CHECK_I32(indices); CHECK_I32(counts);
    CHECK_CONTIG(mma_a); CHECK_CONTIG(mma_b); CHECK_CONTIG(mma_c); CHECK_CONTIG(indices); CHECK_CONTIG(counts);
    TORCH_CHECK((mma_a.dim() == 2 || mma_a.dim() == 3) && mma_b.dim() == 2 && mma_c.dim() == mma_a.dim(),
                "mma_a and mma_c must both be 2D ([M, .]) or 3D ([B, M, .]) tensors, mma_b 2D");
    const int64_t B = mma_a.dim() == 3 ? mma_a.size(0) : 1;
    const int64_t M = mma_a.size(-2), F = mma_a.size(-1), N2 = mma_b.size(1);
    TORCH_CHECK(B >= 1, "the batch size must be at least 1");
    TORCH_CHECK(mma_b.size(0) == F && mma_c.size(-2) == M && mma_c.size(-1) == N2 && mma_c.numel() == B * M * N2,
                "shape mismatch (mma_b must be [F, N2], mma_c [M, N2], or [B, M, N2] with the batch size of mma_a)");
    c10::DeviceGuard guard(mma_a.device());
    TORCH_CHECK(indices.numel() == B * groups_of(M) * F && counts.numel() == B * groups_of(M),
                "indices must be [ceil(M/128), F], counts [ceil(M/128)] ([B, ceil(M/128), F] and [B, ceil(M/128)] with the batch size of mma_a)");
    TORCH_CHECK(B * groups_of(M) <= 65535, "B * ceil(M/128) groups must not exceed 65535 (got ", B * groups_of(M), ")");
    if (B > 1) {
        check(chipmunk_csp_mlp_mm2_w8_batched(mma_a.data_ptr(), mma_b.data_ptr(), scale_b.data_ptr<float>(), mma_c.data_ptr(),
                                              indices.data_ptr<int>(), counts.data_ptr<int>(), (int)M, (int)F, (int)N2, (int)B,
                                              cur_stream(mma_a)),
              "csp_mlp_mm2_w8");
        return;
    }
    check(chipmunk_csp_mlp_mm2_w8(mma_a.data_ptr(), mma_b.data_ptr(), scale_b.data_ptr<float>(), mma_c.data_ptr(), indices.data_ptr<int>(),
                                  counts.data_ptr<int>(), (int)M, (int)F, (int)N2, cur_stream(mma_a)),
          "csp_mlp_mm2_w8");
}

// ---------------------------------------------------------------------------------- indexed IO
// reference csrc/indexed_io/copy_indices.cu:82-154
void copy_indices(at::Tensor bmfc1, at::Tensor bm_mid_cache, at::Tensor sp_inds, at::Tensor sp_counts) {
    CHECK_DEV(bmfc1); CHECK_DEV(bm_mid_cache); CHECK_DEV(sp_inds); CHECK_DEV(sp_counts);
    CHECK_CONTIG(bmfc1); CHECK_CONTIG(bm_mid_cache); CHECK_CONTIG(sp_inds); CHECK_CONTIG(sp_counts);
    TORCH_CHECK(bmfc1.dim() == 3 && bm_mid_cache.dim() == 3, "bmfc1 and bm_mid_cache must be 3D [B, M*R, F]");
    TORCH_CHECK(sp_inds.dim() == 3 && sp_counts.dim() == 2, "sp_inds must be [B, M, F] and sp_counts [B, M]");
    CHECK_I32(sp_inds); CHECK_I32(sp_counts);
    TORCH_CHECK(bmfc1.scalar_type() == bm_mid_cache.scalar_type(), "bmfc1 and bm_mid_cache must have the same dtype");
    TORCH_CHECK(bmfc1.sizes() == bm_mid_cache.sizes(), "bmfc1 and bm_mid_cache must have the same shape");
    const auto st = bmfc1.scalar_type();
    TORCH_CHECK(st == at::kBFloat16 || st == at::kHalf || st == at::kFloat, "Unsupported dtype for copy_indices");
    const int64_t B = bmfc1.size(0), MR = bmfc1.size(1), F = bmfc1.size(2), M = sp_counts.size(1);
    TORCH_CHECK(M > 0 && MR % M == 0 && sp_inds.size(1) == M && sp_inds.size(2) == F, "inconsistent shapes");
    c10::DeviceGuard guard(bmfc1.device());
    check(chipmunk_copy_indices(bmfc1.data_ptr(), bm_mid_cache.data_ptr(), sp_inds.data_ptr<int>(),
                                sp_counts.data_ptr<int>(), (int)B, (int)M, (int)(MR / M), (int)F,
                                (int)bmfc1.element_size(), cur_stream(bmfc1)),
          "copy_indices");
}

// reference csrc/indexed_io/topk_indices.cu:145-218
void topk_indices(at::Tensor activation, at::Tensor indices, at::Tensor counts, double sparsity_amount,
                  int64_t multiple_of, double random_amount) {
    CHECK_DEV(activation); CHECK_DEV(indices); CHECK_DEV(counts);
    CHECK_CONTIG(activation); CHECK_CONTIG(indices); CHECK_CONTIG(counts);
    TORCH_CHECK(activation.dim() == 3, "activation must be [batch, rows, cols]");
    CHECK_I32(indices); CHECK_I32(counts);
    TORCH_CHECK(indices.sizes() == activation.sizes(), "indices must have the shape of activation");
    TORCH_CHECK(counts.numel() == activation.size(0) * activation.size(1), "counts must be [batch, rows]");
    int dtype;
    switch (activation.scalar_type()) {
        case at::kBFloat16: dtype = CHIPMUNK_DTYPE_BF16; break;
        case at::kHalf: dtype = CHIPMUNK_DTYPE_FP16; break;
        case at::kFloat: dtype = CHIPMUNK_DTYPE_FP32; break;
        default: TORCH_CHECK(false, "Unsupported dtype for topk_indices");
    }
    c10::DeviceGuard guard(activation.device());
    check(chipmunk_topk_indices(activation.data_ptr(), dtype, indices.data_ptr<int>(), counts.data_ptr<int>(),
                                (int)(activation.size(0) * activation.size(1)), (int)activation.size(2),
                                sparsity_amount, (int)multiple_of, random_amount, cur_stream(activation)),
          "topk_indices");
}

// fused |activation - cache| -> topk_indices -> copy_indices (reference modules/mlp.py:70-85 with bm == mbm)
void topk_delta_indices(at::Tensor activation, at::Tensor cache, at::Tensor indices, at::Tensor counts,
                        double sparsity_amount, int64_t multiple_of, double random_amount) {
    CHECK_DEV(activation); CHECK_DEV(cache); CHECK_DEV(indices); CHECK_DEV(counts);
    CHECK_CONTIG(activation); CHECK_CONTIG(cache); CHECK_CONTIG(indices); CHECK_CONTIG(counts);
    TORCH_CHECK(activation.dim() == 3 && cache.sizes() == activation.sizes(), "activation and cache must be [batch, rows, cols]");
    TORCH_CHECK(cache.scalar_type() == activation.scalar_type(), "activation and cache must have the same dtype");
    CHECK_I32(indices); CHECK_I32(counts);
    TORCH_CHECK(indices.sizes() == activation.sizes(), "indices must have the shape of activation");
    TORCH_CHECK(counts.numel() == activation.size(0) * activation.size(1), "counts must be [batch, rows]");
    int dtype;
    switch (activation.scalar_type()) {
        case at::kBFloat16: dtype = CHIPMUNK_DTYPE_BF16; break;
        case at::kHalf: dtype = CHIPMUNK_DTYPE_FP16; break;
        case at::kFloat: dtype = CHIPMUNK_DTYPE_FP32; break;
        default: TORCH_CHECK(false, "Unsupported dtype for topk_delta_indices");
    }
    c10::DeviceGuard guard(activation.device());
    check(chipmunk_topk_delta_indices(activation.data_ptr(), cache.data_ptr(), dtype, indices.data_ptr<int>(),
                                      counts.data_ptr<int>(), (int)(activation.size(0) * activation.size(1)),
                                      (int)activation.size(2), sparsity_amount, (int)multiple_of, random_amount,
                                      cur_stream(activation)),
          "topk_delta_indices");
}

// topk_indices / topk_delta_indices with a column count per row from the row's mass (mlp.top_p; not in the reference)
static void topk_p_common(const char *who, const at::Tensor &activation, const at::Tensor *cache, const at::Tensor &indices,
                          const at::Tensor &counts, double sparsity_amount, double top_p, double min_keys, int64_t multiple_of,
                          double random_amount) {
    CHECK_DEV(activation); CHECK_DEV(indices); CHECK_DEV(counts);
    CHECK_CONTIG(activation); CHECK_CONTIG(indices); CHECK_CONTIG(counts);
    TORCH_CHECK(activation.dim() == 3, who, ": activation must be [batch, rows, cols]");
    if (cache) {
        TORCH_CHECK(cache->is_cuda() && cache->is_contiguous(), who, ": cache must be a contiguous GPU tensor");
        TORCH_CHECK(cache->sizes() == activation.sizes() && cache->scalar_type() == activation.scalar_type(), who,
                    ": cache must have the shape and dtype of activation");
    }
    CHECK_I32(indices); CHECK_I32(counts);
    TORCH_CHECK(indices.sizes() == activation.sizes(), who, ": indices must have the shape of activation");
    TORCH_CHECK(counts.numel() == activation.size(0) * activation.size(1), who, ": counts must be [batch, rows]");
    int dtype;
    switch (activation.scalar_type()) {
        case at::kBFloat16: dtype = CHIPMUNK_DTYPE_BF16; break;
        case at::kHalf: dtype = CHIPMUNK_DTYPE_FP16; break;
        case at::kFloat: dtype = CHIPMUNK_DTYPE_FP32; break;
        default: TORCH_CHECK(false, "Unsupported dtype for ", who);
    }
    c10::DeviceGuard guard(activation.device());
    const int rows = (int)(activation.size(0) * activation.size(1)), cols = (int)activation.size(2);
    if (cache)
        check(chipmunk_topk_delta_indices_p(activation.data_ptr(), cache->data_ptr(), dtype, indices.data_ptr<int>(), counts.data_ptr<int>(),
                                            rows, cols, sparsity_amount, top_p, min_keys, (int)multiple_of, random_amount,
                                            cur_stream(activation)), who);
    else
        check(chipmunk_topk_indices_p(activation.data_ptr(), dtype, indices.data_ptr<int>(), counts.data_ptr<int>(), rows, cols,
                                      sparsity_amount, top_p, min_keys, (int)multiple_of, random_amount, cur_stream(activation)), who);
}

void topk_indices_p(at::Tensor activation, at::Tensor indices, at::Tensor counts, double sparsity_amount, double top_p,
                    double min_keys, int64_t multiple_of, double random_amount) {
    topk_p_common("topk_indices_p", activation, nullptr, indices, counts, sparsity_amount, top_p, min_keys, multiple_of, random_amount);
}

void topk_delta_indices_p(at::Tensor activation, at::Tensor cache, at::Tensor indices, at::Tensor counts, double sparsity_amount,
                          double top_p, double min_keys, int64_t multiple_of, double random_amount) {
    topk_p_common("topk_delta_indices_p", activation, &cache, indices, counts, sparsity_amount, top_p, min_keys, multiple_of, random_amount);
}

// topk_delta_indices over rows_per_group block-mean rows per 128-row group (mlp.fused_group_topk_delta; not in the reference): the score of
// a column is the fp32 sum of the rows' |delta|, rounded once; `top_p` null: the top-k selection, otherwise the _p one
static void topk_group_common(const char *who, const at::Tensor &activation, const at::Tensor &cache, const at::Tensor &indices,
                              const at::Tensor &counts, int64_t rows_per_group, double sparsity_amount, const double *top_p, double min_keys,
                              int64_t multiple_of, double random_amount) {
    CHECK_DEV(activation); CHECK_DEV(cache); CHECK_DEV(indices); CHECK_DEV(counts);
    CHECK_CONTIG(activation); CHECK_CONTIG(cache); CHECK_CONTIG(indices); CHECK_CONTIG(counts);
    TORCH_CHECK(activation.dim() == 3 && cache.sizes() == activation.sizes(), who, ": activation and cache must be [batch, rows, cols]");
    TORCH_CHECK(cache.scalar_type() == activation.scalar_type(), who, ": activation and cache must have the same dtype");
    CHECK_I32(indices); CHECK_I32(counts);
    TORCH_CHECK(rows_per_group >= 1 && rows_per_group <= 64, who, ": rows_per_group must be in [1, 64] (got ", rows_per_group, ")");
    const int64_t B = activation.size(0), rows = activation.size(1), F = activation.size(2);
    TORCH_CHECK(rows >= 1 && rows < (1ll << 31) && F < (1ll << 31), who, ": activation must have 1 .. 2^31 - 1 rows and columns");
    const int64_t G = (rows + rows_per_group - 1) / rows_per_group;
    TORCH_CHECK(indices.dim() == 3 && indices.size(0) == B && indices.size(1) == G && indices.size(2) == F, who,
                ": indices must be [batch, ceil(rows / rows_per_group), cols] = [", B, ", ", G, ", ", F, "]");
    TORCH_CHECK(counts.dim() == 2 && counts.size(0) == B && counts.size(1) == G, who, ": counts must be [batch, ceil(rows / rows_per_group)]");
    TORCH_CHECK(B * G < (1ll << 31), who, ": too many groups");
    int dtype;
    switch (activation.scalar_type()) {
        case at::kBFloat16: dtype = CHIPMUNK_DTYPE_BF16; break;
        case at::kHalf: dtype = CHIPMUNK_DTYPE_FP16; break;
        case at::kFloat: dtype = CHIPMUNK_DTYPE_FP32; break;
        default: TORCH_CHECK(false, "Unsupported dtype for ", who);
    }
    c10::DeviceGuard guard(activation.device());
    if (top_p)
        check(chipmunk_topk_group_delta_indices_p(activation.data_ptr(), cache.data_ptr(), dtype, indices.data_ptr<int>(), counts.data_ptr<int>(),
                                                  (int)B, (int)rows, (int)rows_per_group, (int)F, sparsity_amount, *top_p, min_keys,
                                                  (int)multiple_of, random_amount, cur_stream(activation)), who);
    else
        check(chipmunk_topk_group_delta_indices(activation.data_ptr(), cache.data_ptr(), dtype, indices.data_ptr<int>(), counts.data_ptr<int>(),
                                                (int)B, (int)rows, (int)rows_per_group, (int)F, sparsity_amount, (int)multiple_of,
                                                random_amount, cur_stream(activation)), who);
}

void topk_group_delta_indices(at::Tensor activation, at::Tensor cache, at::Tensor indices, at::Tensor counts, int64_t rows_per_group,
                              double sparsity_amount, int64_t multiple_of, double random_amount) {
    topk_group_common("topk_group_delta_indices", activation, cache, indices, counts, rows_per_group, sparsity_amount, nullptr, 0.0,
                      multiple_of, random_amount);
}

void topk_group_delta_indices_p(at::Tensor activation, at::Tensor cache, at::Tensor indices, at::Tensor counts, int64_t rows_per_group,
                                double sparsity_amount, double top_p, double min_keys, int64_t multiple_of, double random_amount) {
    topk_group_common("topk_group_delta_indices_p", activation, cache, indices, counts, rows_per_group, sparsity_amount, &top_p, min_keys,
                      multiple_of, random_amount);
}

// reference csrc/indexed_io/mask_to_indices.cu:92-143
std::vector<at::Tensor> mask_to_indices(at::Tensor mask, int64_t multiple_of, int64_t pad_to_multiple_of) {
    TORCH_CHECK(mask.dim() == 4, "mask must be 4-dimensional [b, h, m, n]");
    TORCH_CHECK(mask.scalar_type() == at::kBool, "mask must be bool type");
    CHECK_DEV(mask);
    TORCH_CHECK(multiple_of > 0 && pad_to_multiple_of > 0, "multiple_of and pad_to_multiple_of must be positive");
    mask = mask.contiguous();
    const int64_t b = mask.size(0), h = mask.size(1), m = mask.size(2), n = mask.size(3);
    const int64_t pad_n = ((n + pad_to_multiple_of - 1) / pad_to_multiple_of) * pad_to_multiple_of;
    c10::DeviceGuard guard(mask.device());
    at::Tensor indices = at::empty({b, h, m, pad_n}, mask.options().dtype(at::kInt));
    at::Tensor counts = at::empty({b, h, m}, mask.options().dtype(at::kInt));
    check(chipmunk_mask_to_indices(mask.data_ptr(), indices.data_ptr<int>(), counts.data_ptr<int>(), b * h * m, (int)n,
                                   (int)pad_n, (int)multiple_of, cur_stream(mask)),
          "mask_to_indices");
    return {indices, counts};
}

// fused bitunpack + mask_to_indices: `packed` is ops.bitpack's output for a [b,h,m,n] mask
std::vector<at::Tensor> packed_mask_to_indices(at::Tensor packed, at::IntArrayRef shape, int64_t multiple_of,
                                               int64_t pad_to_multiple_of) {
    TORCH_CHECK(packed.scalar_type() == at::kByte && packed.is_contiguous(), "packed must be a contiguous uint8 tensor");
    CHECK_DEV(packed);
    TORCH_CHECK(shape.size() == 4, "shape must be [b, h, m, n]");
    const int64_t b = shape[0], h = shape[1], m = shape[2], n = shape[3];
    TORCH_CHECK(n % 8 == 0, "n must be a multiple of 8");
    TORCH_CHECK(packed.numel() * 8 >= b * h * m * n, "packed is too short for the given shape");
    const int64_t pad_n = ((n + pad_to_multiple_of - 1) / pad_to_multiple_of) * pad_to_multiple_of;
    c10::DeviceGuard guard(packed.device());
    at::Tensor indices = at::empty({b, h, m, pad_n}, packed.options().dtype(at::kInt));
    at::Tensor counts = at::empty({b, h, m}, packed.options().dtype(at::kInt));
    check(chipmunk_packed_mask_to_indices(packed.data_ptr(), indices.data_ptr<int>(), counts.data_ptr<int>(),
                                          b * h * m, (int)n, (int)pad_n, (int)multiple_of, cur_stream(packed)),
          "packed_mask_to_indices");
    return {indices, counts};
}

// x.transpose(-1, -2).contiguous() for 16-bit dtypes in one HBM-rate kernel (reference modules/mlp.py:56)
at::Tensor transpose_last2(at::Tensor x) {
    CHECK_DEV(x);
    TORCH_CHECK(x.dim() >= 2 && x.element_size() == 2, "transpose_last2: need a >=2-D tensor of a 16-bit dtype");
    x = x.contiguous();
    const int64_t R = x.size(-2), C = x.size(-1), B = x.numel() / (R * C);
    auto sizes = x.sizes().vec();
    std::swap(sizes[sizes.size() - 1], sizes[sizes.size() - 2]);
    c10::DeviceGuard guard(x.device());
    at::Tensor out = at::empty(sizes, x.options());
    check(chipmunk_transpose16(x.data_ptr(), out.data_ptr(), (int)B, (int)R, (int)C, cur_stream(x)), "transpose_last2");
    return out;
}

// transpose_last2 into rows of `ld` >= R elements: [..., C, ld] with elements [R, ld) of every row zero; [..., :R] is the transpose (the
// activation cache of a token count that is not a multiple of 8: the MLP operators take that view, its owner keeps the whole tensor)
at::Tensor transpose_last2_pitched(at::Tensor x, int64_t ld) {
    CHECK_DEV(x);
    TORCH_CHECK(x.dim() >= 2 && x.element_size() == 2, "transpose_last2_pitched: need a >=2-D tensor of a 16-bit dtype");
    x = x.contiguous();
    const int64_t R = x.size(-2), C = x.size(-1), B = x.numel() / (R * C);
    TORCH_CHECK(ld >= R, "transpose_last2_pitched: ld must be at least the row count");
    auto sizes = x.sizes().vec();
    sizes[sizes.size() - 2] = C;
    sizes[sizes.size() - 1] = ld;
    c10::DeviceGuard guard(x.device());
    at::Tensor out = at::empty(sizes, x.options());
    check(chipmunk_transpose16_pitched(x.data_ptr(), out.data_ptr(), (int)B, (int)R, (int)C, (int)ld, cur_stream(x)), "transpose_last2_pitched");
    return out;
}

// [..., R, C] -> [..., ceil(R / 128), C, 128] for a 16-bit dtype: out[..., g, c, r] = x[..., g * 128 + r, c], the rows of the last group at
// or past R zero -- the group-major activation cache of a full step
at::Tensor transpose_to_groups(at::Tensor x) {
    CHECK_DEV(x);
    TORCH_CHECK(x.dim() >= 2 && x.element_size() == 2, "transpose_to_groups: need a >=2-D tensor of a 16-bit dtype");
    x = x.contiguous();
    const int64_t R = x.size(-2), C = x.size(-1);
    TORCH_CHECK(R > 0 && C > 0, "transpose_to_groups: the last two dimensions must not be empty");
    const int64_t B = x.numel() / (R * C);
    auto sizes = x.sizes().vec();
    sizes[sizes.size() - 2] = groups_of(R);
    sizes[sizes.size() - 1] = C;
    sizes.push_back(128);
    c10::DeviceGuard guard(x.device());
    at::Tensor out = at::empty(sizes, x.options());
    check(chipmunk_transpose16_groups(x.data_ptr(), out.data_ptr(), (int)B, (int)R, (int)C, cur_stream(x)), "transpose_to_groups");
    return out;
}

// [b, n, c] -> [b, n / mbm, c] mean over consecutive row blocks (reference modules/mlp.py:11-16) in one HBM-rate kernel, bf16
at::Tensor block_mean(at::Tensor x, int64_t mbm) {
    CHECK_DEV(x);
    TORCH_CHECK(x.dim() == 3 && x.scalar_type() == at::kBFloat16, "block_mean: need a [b, n, c] bfloat16 tensor");
    TORCH_CHECK(mbm > 0 && x.size(1) > 0, "block_mean: mbm and n must be positive");
    x = x.contiguous();
    c10::DeviceGuard guard(x.device());
    const int64_t n = x.size(1), blocks = (n + mbm - 1) / mbm;
    at::Tensor out = at::empty({x.size(0), blocks, x.size(2)}, x.options());
    if (n % mbm == 0) {
        check(chipmunk_block_mean(x.data_ptr(), out.data_ptr(), x.size(0) * n, (int)x.size(2), (int)mbm, cur_stream(x)), "block_mean");
    } else {   // a ragged last block (the mean over the rows present) ends every batch entry: one launch each
        for (int64_t b = 0; b < x.size(0); ++b)
            check(chipmunk_block_mean_ragged(x[b].data_ptr(), out[b].data_ptr(), n, (int)x.size(2), (int)mbm, cur_stream(x)), "block_mean");
    }
    return out;
}

// F8Linear.quantize_input as one kernel: (x * scale).clamp(-max, max).to(float8_e4m3fn), same roundings
at::Tensor quantize_fp8(at::Tensor x, at::Tensor scale, double max_value) {
    CHECK_DEV(x); CHECK_DEV(scale);
    TORCH_CHECK(x.scalar_type() == at::kBFloat16, "quantize_fp8: x must be bfloat16");
    TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.numel() == 1, "quantize_fp8: scale must be a one-element float32 tensor");
    TORCH_CHECK(x.numel() % 8 == 0, "quantize_fp8: the element count must be a multiple of 8");
    x = x.contiguous();
    c10::DeviceGuard guard(x.device());
    at::Tensor out = at::empty(x.sizes(), x.options().dtype(at::kFloat8_e4m3fn));
    check(chipmunk_quantize_fp8(x.data_ptr(), scale.data_ptr<float>(), out.data_ptr(), x.numel(), (float)max_value, cur_stream(x)), "quantize_fp8");
    return out;
}

// F8Linear.quantize_input_rowwise as one kernel: x [..., K] bf16 -> (e4m3 [..., K], float32 [...] reciprocal scales), one scale per row
std::vector<at::Tensor> quantize_fp8_rowwise(at::Tensor x, double max_value) {
    CHECK_DEV(x);
    TORCH_CHECK(x.scalar_type() == at::kBFloat16, "quantize_fp8_rowwise: x must be bfloat16");
    TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0 && x.size(-1) % 16 == 0 && x.size(-1) <= CHIPMUNK_QUANTIZE_ROWWISE_MAX_K,
                "quantize_fp8_rowwise: the last dimension must be a positive multiple of 16, at most ", CHIPMUNK_QUANTIZE_ROWWISE_MAX_K);
    x = x.contiguous();
    c10::DeviceGuard guard(x.device());
    const int64_t K = x.size(-1), rows = x.numel() / K;
    at::Tensor out = at::empty(x.sizes(), x.options().dtype(at::kFloat8_e4m3fn));
    at::Tensor recip = at::empty(x.sizes().slice(0, x.dim() - 1), x.options().dtype(at::kFloat));
    check(chipmunk_quantize_fp8_rowwise(x.data_ptr(), out.data_ptr(), recip.data_ptr<float>(), rows, (int)K, (float)max_value, cur_stream(x)),
          "quantize_fp8_rowwise");
    return {out, recip};
}

// ascending-order variant of (packed_)mask_to_indices (same set / counts / padding; see chipmunk_hip.h)
std::vector<at::Tensor> mask_to_sorted_indices(at::Tensor mask, at::IntArrayRef shape, int64_t multiple_of,
                                               int64_t pad_to_multiple_of) {
    CHECK_DEV(mask);
    const bool packed = mask.scalar_type() == at::kByte;
    TORCH_CHECK(packed || mask.scalar_type() == at::kBool, "mask must be bool, or uint8 bit-packed with a shape");
    mask = mask.contiguous();
    std::vector<int64_t> shp = packed ? shape.vec() : mask.sizes().vec();
    TORCH_CHECK(shp.size() == 4, "shape must be [b, h, m, n]");
    const int64_t b = shp[0], h = shp[1], m = shp[2], n = shp[3];
    if (packed) TORCH_CHECK(n % 8 == 0 && mask.numel() * 8 >= b * h * m * n, "bad packed mask");
    const int64_t pad_n = ((n + pad_to_multiple_of - 1) / pad_to_multiple_of) * pad_to_multiple_of;
    c10::DeviceGuard guard(mask.device());
    at::Tensor indices = at::empty({b, h, m, pad_n}, mask.options().dtype(at::kInt));
    at::Tensor counts = at::empty({b, h, m}, mask.options().dtype(at::kInt));
    check(chipmunk_mask_to_sorted_indices(mask.data_ptr(), packed ? 1 : 0, indices.data_ptr<int>(),
                                          counts.data_ptr<int>(), b * h * m, (int)n, (int)pad_n, (int)multiple_of,
                                          cur_stream(mask)),
          "mask_to_sorted_indices");
    return {indices, counts};
}

// addition: the rows of (packed_)mask_to_indices / mask_to_sorted_indices followed by compact_indices, without the padded [b, h, m, pad_n]
// tensor between them: {flat, offsets, counts}.  The size of flat depends on the mask, hence one host sync and no fake kernel.
std::vector<at::Tensor> mask_to_ragged_indices(at::Tensor mask, at::IntArrayRef shape, int64_t multiple_of, int64_t pad_to_multiple_of,
                                               bool sorted) {
    CHECK_DEV(mask);
    const bool packed = mask.scalar_type() == at::kByte;
    TORCH_CHECK(packed || mask.scalar_type() == at::kBool, "mask must be bool, or uint8 bit-packed with a shape");
    TORCH_CHECK(multiple_of > 0 && pad_to_multiple_of > 0, "multiple_of and pad_to_multiple_of must be positive");
    mask = mask.contiguous();
    std::vector<int64_t> shp = packed ? shape.vec() : mask.sizes().vec();
    TORCH_CHECK(shp.size() == 4, "shape must be [b, h, m, n]");
    const int64_t b = shp[0], h = shp[1], m = shp[2], n = shp[3], rows = b * h * m;
    if (packed) TORCH_CHECK(n % 8 == 0 && mask.numel() * 8 >= rows * n, "bad packed mask");
    const int64_t pad_n = ((n + pad_to_multiple_of - 1) / pad_to_multiple_of) * pad_to_multiple_of;
    TORCH_CHECK(n > 0 && pad_n <= INT_MAX, "rows must have between 1 and 2^31 - 1 columns");
    c10::DeviceGuard guard(mask.device());
    at::Tensor counts = at::empty({b, h, m}, mask.options().dtype(at::kInt));
    at::Tensor len = at::empty({rows}, mask.options().dtype(at::kLong));
    check(chipmunk_mask_row_counts(mask.data_ptr(), packed ? 1 : 0, counts.data_ptr<int>(), len.data_ptr<int64_t>(), rows, (int)n,
                                   (int)pad_n, (int)multiple_of, cur_stream(mask)),
          "mask_to_ragged_indices");
    at::Tensor offsets = at::zeros({rows + 1}, len.options());
    if (rows) offsets.narrow(0, 1, rows).copy_(len.cumsum(0));
    const int64_t total = rows ? offsets[rows].item<int64_t>() : 0;      // the one host sync (as compact_indices)
    at::Tensor flat = at::empty({total + 64}, counts.options());
    flat.narrow(0, total, 64).zero_();
    check(chipmunk_mask_to_ragged_indices(mask.data_ptr(), packed ? 1 : 0, sorted ? 1 : 0, offsets.data_ptr<int64_t>(), flat.data_ptr<int>(),
                                          rows, (int)n, (int)multiple_of, cur_stream(mask)),
          "mask_to_ragged_indices");
    return {flat, offsets, counts};
}

// addition: randint + topk + scatter_ + the two mask combines of modules/attn.py:76-82 in one kernel
// dense_colsum_attn + topk_mask without the cs tensor between them (see chipmunk_dense_colsum_topk_mask); falls back to the two
// operators when the fused entry does not apply to the launch
std::vector<at::Tensor> dense_colsum_attn_layout(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor p, bool token_major_o);
// (the `_p` operators: `mass` set, `top_p` / `k_min` the per-row count of chipmunk_topk_mask_p with k as the cap)
static at::Tensor topk_mask_impl(at::Tensor cs, int64_t k, bool mass, double top_p, int64_t k_min, double random_amount,
                                 const c10::optional<at::Tensor> &groups, const c10::optional<at::Tensor> &static_mask,
                                 const OptTensor &k_lens = c10::nullopt);
static std::vector<at::Tensor> dense_colsum_topk_mask_impl(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor p, int64_t k_top, bool mass, double top_p,
                                                           int64_t k_min, double random_amount, const c10::optional<at::Tensor> &groups,
                                                           const c10::optional<at::Tensor> &static_mask, bool token_major_o,
                                                           const OptTensor &k_lens = c10::nullopt) {
    const int32_t *kl = klens_ptr(k_lens, q, q.dim() == 4 ? q.size(0) : 0);
    if (mass) TORCH_CHECK(top_p > 0.0 && top_p <= 1.0 && k_min >= 0, "top_p must be in (0, 1] and k_min >= 0 (got ", top_p, ", ", k_min, ")");
    CHECK_DEV(q); CHECK_DEV(k); CHECK_DEV(v); CHECK_DEV(p);
    CHECK_BF16(q); CHECK_BF16(k); CHECK_BF16(v);
    const bool shapes_ok = q.dim() == 4 && k.dim() == 4 && v.dim() == 4 && q.size(3) == 128 && q.stride(3) == 1 && k.stride(3) == 1 &&
                           v.stride(3) == 1 && p.scalar_type() == at::kFloat && p.is_contiguous();
    if (shapes_ok) {
        const int64_t B = q.size(0), H = q.size(1), Nq = q.size(2), Nk = k.size(2), G = (Nq + 191) / 192;
        const void *st = nullptr, *gf = nullptr;
        int64_t st_stride = 0, st_rows = 1;
        at::Tensor stc, gfc;
        bool ok = p.numel() == B * H * Nq;
        if (ok && static_mask.has_value() && static_mask->defined()) {
            stc = *static_mask;
            ok = stc.is_cuda() && stc.scalar_type() == at::kBool && stc.dim() == 4 && stc.size(3) == Nk && stc.size(2) == G && stc.size(1) == H &&
                 (stc.size(0) == 1 || stc.size(0) == B) && stc.stride(3) == 1 && stc.stride(1) == G * stc.stride(2) &&
                 (stc.size(0) == 1 || stc.stride(0) == H * stc.stride(1));
            if (ok) st = stc.data_ptr(), st_stride = stc.stride(2), st_rows = stc.size(0) * H * G;
        }
        if (ok && groups.has_value() && groups->defined()) {
            gfc = *groups;
            ok = gfc.is_cuda() && gfc.scalar_type() == at::kBool && gfc.dim() == 4 && gfc.size(3) == 1 && gfc.size(2) == G && gfc.size(1) == H &&
                 (gfc.size(0) == 1 || gfc.size(0) == B);
            if (ok) {
                gfc = gfc.expand({B, H, G, 1}).contiguous();
                gf = gfc.data_ptr();
            }
        }
        if (ok) {
            c10::DeviceGuard guard(q.device());
            at::Tensor o = alloc_o(q, q, token_major_o);
            const int64_t os[3] = {o.stride(0), o.stride(1), o.stride(2)};
            at::Tensor l = at::empty({B, H, Nq, 1}, q.options().dtype(at::kFloat));
            at::Tensor mask = at::empty({B, H, G, Nk}, q.options().dtype(at::kBool));
            const int64_t qs[3] = {q.stride(0), q.stride(1), q.stride(2)}, ks[3] = {k.stride(0), k.stride(1), k.stride(2)},
                          vs[3] = {v.stride(0), v.stride(1), v.stride(2)};
            const int rc = mass ? chipmunk_dense_colsum_topk_mask_p_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), qs, ks, vs, p.data_ptr<float>(), o.data_ptr(),
                                                                           os, l.data_ptr<float>(), kl, (int)B, (int)H, (int)Nq, (int)Nk, st, st_stride, (int)st_rows, gf,
                                                                           mask.data_ptr(), (int)k_top, random_amount, top_p, (int)(k_min > Nk ? Nk : k_min), cur_stream(q))
                                : chipmunk_dense_colsum_topk_mask_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), qs, ks, vs, p.data_ptr<float>(), o.data_ptr(),
                                                           os, l.data_ptr<float>(), kl, (int)B, (int)H, (int)Nq, (int)Nk, st, st_stride, (int)st_rows, gf,
                                                           mask.data_ptr(), (int)k_top, random_amount, cur_stream(q));
            if (rc == CHIPMUNK_OK) return {o, mask, l};
            if (rc != CHIPMUNK_ERR_UNSUPPORTED) check(rc, "dense_colsum_topk_mask");
        }
    }
    auto ocl = dense_colsum_attn_klens(q, k, v, p, token_major_o, k_lens);
    at::Tensor cs = ocl[1];
    const int64_t Nk = k.size(2), G = (q.size(2) + 191) / 192;
    if (cs.size(-1) != Nk || cs.size(-2) != G) cs = cs.slice(-2, 0, G).slice(-1, 0, Nk);
    return {ocl[0], topk_mask_impl(cs, k_top, mass, top_p, k_min, random_amount, groups, static_mask, k_lens), ocl[2]};
}

std::vector<at::Tensor> dense_colsum_topk_mask_varlen(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor p, at::Tensor k_lens, int64_t k_top,
                                                      double random_amount, const c10::optional<at::Tensor> &groups,
                                                      const c10::optional<at::Tensor> &static_mask, bool token_major_o) {
    return dense_colsum_topk_mask_impl(q, k, v, p, k_top, false, 0.0, 0, random_amount, groups, static_mask, token_major_o, k_lens);
}

std::vector<at::Tensor> dense_colsum_topk_mask_p_varlen(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor p, at::Tensor k_lens, int64_t k_top,
                                                        double top_p, int64_t k_min, double random_amount, const c10::optional<at::Tensor> &groups,
                                                        const c10::optional<at::Tensor> &static_mask, bool token_major_o) {
    return dense_colsum_topk_mask_impl(q, k, v, p, k_top, true, top_p, k_min, random_amount, groups, static_mask, token_major_o, k_lens);
}

std::vector<at::Tensor> dense_colsum_topk_mask(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor p, int64_t k_top, double random_amount,
                                               const c10::optional<at::Tensor> &groups, const c10::optional<at::Tensor> &static_mask,
                                               bool token_major_o) {
    return dense_colsum_topk_mask_impl(q, k, v, p, k_top, false, 0.0, 0, random_amount, groups, static_mask, token_major_o);
}

std::vector<at::Tensor> dense_colsum_topk_mask_p(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor p, int64_t k_top, double top_p, int64_t k_min,
                                                 double random_amount, const c10::optional<at::Tensor> &groups,
                                                 const c10::optional<at::Tensor> &static_mask, bool token_major_o) {
    return dense_colsum_topk_mask_impl(q, k, v, p, k_top, true, top_p, k_min, random_amount, groups, static_mask, token_major_o);
}

static at::Tensor topk_mask_impl(at::Tensor cs, int64_t k, bool mass, double top_p, int64_t k_min, double random_amount,
                                 const c10::optional<at::Tensor> &groups, const c10::optional<at::Tensor> &static_mask,
                                 const OptTensor &k_lens) {
    CHECK_DEV(cs); CHECK_BF16(cs);
    TORCH_CHECK(cs.dim() == 4 && cs.stride(3) == 1, "cs must be [B, H, G, N] with a contiguous last dim");
    const int64_t B = cs.size(0), H = cs.size(1), G = cs.size(2), N = cs.size(3);
    const int32_t *kl = klens_ptr(k_lens, cs, B);
    // rows must be addressable with one stride: collapse (B, H, G) or copy
    if (!(cs.stride(1) == G * cs.stride(2) && (B == 1 || cs.stride(0) == H * cs.stride(1)))) cs = cs.contiguous();
    const int64_t rows = B * H * G;
    c10::DeviceGuard guard(cs.device());
    at::Tensor mask = at::empty({B, H, G, N}, cs.options().dtype(at::kBool));
    const void *st = nullptr, *gf = nullptr;
    int64_t st_stride = 0, st_rows = 1;
    at::Tensor stc, gfc;
    if (static_mask.has_value() && static_mask->defined()) {
        stc = *static_mask;
        CHECK_DEV(stc);
        TORCH_CHECK(stc.scalar_type() == at::kBool && stc.dim() == 4 && stc.size(3) == N && stc.size(2) == G &&
                    stc.size(1) == H && (stc.size(0) == 1 || stc.size(0) == B), "static_mask must be bool [1|B, H, G, N]");
        if (!(stc.stride(3) == 1 && stc.stride(1) == G * stc.stride(2) && (stc.size(0) == 1 || stc.stride(0) == H * stc.stride(1))))
            stc = stc.contiguous();
        st = stc.data_ptr(), st_stride = stc.stride(2), st_rows = stc.size(0) * H * G;
    }
    if (groups.has_value() && groups->defined()) {
        gfc = *groups;
        CHECK_DEV(gfc);
        TORCH_CHECK(gfc.scalar_type() == at::kBool && gfc.dim() == 4 && gfc.size(3) == 1 && gfc.size(2) == G &&
                    gfc.size(1) == H && (gfc.size(0) == 1 || gfc.size(0) == B), "groups must be bool [1|B, H, G, 1]");
        gfc = gfc.expand({B, H, G, 1}).contiguous();
        gf = gfc.data_ptr();
    }
    if (mass)
        check(chipmunk_topk_mask_p_varlen(cs.data_ptr(), cs.stride(2), st, st_stride, (int)st_rows, gf, mask.data_ptr(), kl, (int)(H * G),
                                          (int)rows, (int)N, (int)k, random_amount, top_p, (int)(k_min > N ? N : k_min), cur_stream(cs)),
              "topk_mask_p");
    else
        check(chipmunk_topk_mask_varlen(cs.data_ptr(), cs.stride(2), st, st_stride, (int)st_rows, gf, mask.data_ptr(), kl, (int)(H * G),
                                        (int)rows, (int)N, (int)k, random_amount, cur_stream(cs)),
              "topk_mask");
    return mask;
}

at::Tensor topk_mask_varlen(at::Tensor cs, at::Tensor k_lens, int64_t k, double random_amount, const c10::optional<at::Tensor> &groups,
                            const c10::optional<at::Tensor> &static_mask) {
    return topk_mask_impl(cs, k, false, 0.0, 0, random_amount, groups, static_mask, k_lens);
}

at::Tensor topk_mask_p_varlen(at::Tensor cs, at::Tensor k_lens, int64_t k, double top_p, int64_t k_min, double random_amount,
                              const c10::optional<at::Tensor> &groups, const c10::optional<at::Tensor> &static_mask) {
    return topk_mask_impl(cs, k, true, top_p, k_min, random_amount, groups, static_mask, k_lens);
}

at::Tensor topk_mask(at::Tensor cs, int64_t k, double random_amount, const c10::optional<at::Tensor> &groups,
                     const c10::optional<at::Tensor> &static_mask) {
    return topk_mask_impl(cs, k, false, 0.0, 0, random_amount, groups, static_mask);
}

at::Tensor topk_mask_p(at::Tensor cs, int64_t k, double top_p, int64_t k_min, double random_amount, const c10::optional<at::Tensor> &groups,
                       const c10::optional<at::Tensor> &static_mask) {
    return topk_mask_impl(cs, k, true, top_p, k_min, random_amount, groups, static_mask);
}

// reference src/chipmunk/ops/bitpack.py:4-69 as single kernels
at::Tensor bitpack(at::Tensor mask) {
    TORCH_CHECK(mask.scalar_type() == at::kBool, "mask must be bool type");
    CHECK_DEV(mask);
    mask = mask.contiguous();
    c10::DeviceGuard guard(mask.device());
    at::Tensor packed = at::empty({(mask.numel() + 7) / 8}, mask.options().dtype(at::kByte));
    check(chipmunk_bitpack(mask.data_ptr(), packed.data_ptr(), mask.numel(), cur_stream(mask)), "bitpack");
    return packed;
}
at::Tensor bitunpack(at::Tensor packed, at::IntArrayRef shape) {
    TORCH_CHECK(packed.scalar_type() == at::kByte && packed.is_contiguous(), "packed must be a contiguous uint8 tensor");
    CHECK_DEV(packed);
    int64_t n = 1;
    for (auto d : shape) n *= d;
    TORCH_CHECK(packed.numel() * 8 >= n, "packed is too short for the given shape");
    c10::DeviceGuard guard(packed.device());
    at::Tensor mask = at::empty(shape, packed.options().dtype(at::kBool));
    check(chipmunk_bitunpack(packed.data_ptr(), mask.data_ptr(), n, cur_stream(packed)), "bitunpack");
    return mask;
}

// [n, >= 3*heads*128] projection output -> q, k, v [1, heads, n, 128] with q/k RMSNorm (see chipmunk_qkv_split_norm)
std::vector<at::Tensor> qkv_split_norm(at::Tensor qkv, const c10::optional<at::Tensor> &q_weight, const c10::optional<at::Tensor> &k_weight,
                                       int64_t heads, double eps, const c10::optional<at::Tensor> &freqs_cos,
                                       const c10::optional<at::Tensor> &freqs_sin) {
    CHECK_DEV(qkv); CHECK_BF16(qkv);
    TORCH_CHECK(qkv.dim() == 2 && qkv.stride(1) == 1 && qkv.size(1) >= 3 * heads * 128, "qkv_split_norm: qkv must be [n, >= 3*heads*128] with a contiguous last dim");
    const void *qw = nullptr, *kw = nullptr;
    at::Tensor qwc, kwc;
    if (q_weight.has_value() && q_weight->defined()) { qwc = q_weight->contiguous(); CHECK_DEV(qwc); CHECK_BF16(qwc); TORCH_CHECK(qwc.numel() == 128); qw = qwc.data_ptr(); }
    if (k_weight.has_value() && k_weight->defined()) { kwc = k_weight->contiguous(); CHECK_DEV(kwc); CHECK_BF16(kwc); TORCH_CHECK(kwc.numel() == 128); kw = kwc.data_ptr(); }
    const int64_t n = qkv.size(0);
    const float *fc = nullptr, *fs = nullptr;
    int64_t rope_rows = 0;
    at::Tensor fcc, fsc;
    if (freqs_cos.has_value() && freqs_cos->defined()) {
        TORCH_CHECK(freqs_sin.has_value() && freqs_sin->defined(), "qkv_split_norm: freqs_cos without freqs_sin");
        fcc = freqs_cos->contiguous(), fsc = freqs_sin->contiguous();
        CHECK_DEV(fcc); CHECK_DEV(fsc);
        TORCH_CHECK(fcc.scalar_type() == at::kFloat && fsc.scalar_type() == at::kFloat && fcc.dim() == 2 && fcc.size(1) == 128 &&
                    fsc.sizes() == fcc.sizes() && fcc.size(0) <= n, "qkv_split_norm: freqs must be float32 [rows <= n, 128]");
        fc = fcc.data_ptr<float>(), fs = fsc.data_ptr<float>(), rope_rows = fcc.size(0);
    }
    c10::DeviceGuard guard(qkv.device());
    at::Tensor out = at::empty({3, 1, heads, n, 128}, qkv.options());
    check(chipmunk_qkv_split_norm(qkv.data_ptr(), qkv.stride(0), qw, kw, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), n,
                                  (int)heads, (float)eps, fc, fs, rope_rows, cur_stream(qkv)),
          "qkv_split_norm");
    return {out[0], out[1], out[2]};
}

// [B, n, >= parts*heads*128] (or [n, ...]) -> parts x [B, heads, n, 128]: row-wide RMSNorm, weight, rotary per part (see
// chipmunk_split_heads_rownorm); norm_mask / rope_mask: bit p = part p
std::vector<at::Tensor> split_heads_rownorm(at::Tensor x, int64_t heads, int64_t parts, const c10::optional<at::Tensor> &w0,
                                            const c10::optional<at::Tensor> &w1, const c10::optional<at::Tensor> &w2, int64_t norm_mask,
                                            int64_t rope_mask, double eps, const c10::optional<at::Tensor> &freqs_cos,
                                            const c10::optional<at::Tensor> &freqs_sin) {
    CHECK_DEV(x); CHECK_BF16(x);
    TORCH_CHECK(parts >= 1 && parts <= 3 && heads >= 1 && heads <= 64, "split_heads_rownorm: parts must be in 1 .. 3 and heads in 1 .. 64");
    TORCH_CHECK((x.dim() == 2 || x.dim() == 3) && x.stride(-1) == 1 && x.size(-1) >= parts * heads * 128,
                "split_heads_rownorm: x must be [B, n, >= parts*heads*128] or [n, >= parts*heads*128] with a contiguous last dim");
    TORCH_CHECK(norm_mask >= 0 && rope_mask >= 0 && (norm_mask >> parts) == 0 && (rope_mask >> parts) == 0, "split_heads_rownorm: a mask names a part past parts");
    const int64_t B = x.dim() == 3 ? x.size(0) : 1, n = x.size(-2), C = heads * 128;
    TORCH_CHECK(B >= 1, "split_heads_rownorm: empty batch");
    const c10::optional<at::Tensor> *ws[3] = {&w0, &w1, &w2};
    at::Tensor wc[3];
    const void *wp[3] = {nullptr, nullptr, nullptr};
    int wd[3] = {0, 0, 0};
    for (int p = 0; p < 3; ++p) {
        if (!(ws[p]->has_value() && (*ws[p])->defined())) continue;
        TORCH_CHECK(p < parts && (norm_mask >> p & 1), "split_heads_rownorm: weight ", p, " belongs to a part that is not normalised");
        wc[p] = (*ws[p])->contiguous();
        CHECK_DEV(wc[p]);
        TORCH_CHECK((wc[p].scalar_type() == at::kBFloat16 || wc[p].scalar_type() == at::kFloat) && wc[p].numel() == C,
                    "split_heads_rownorm: a weight must be bfloat16 or float32 with heads*128 entries");
        wp[p] = wc[p].data_ptr(), wd[p] = wc[p].scalar_type() == at::kFloat ? 2 : 1;
    }
    const float *fc = nullptr, *fs = nullptr;
    int64_t rope_rows = 0;
    at::Tensor fcc, fsc;
    const bool has_cos = freqs_cos.has_value() && freqs_cos->defined(), has_sin = freqs_sin.has_value() && freqs_sin->defined();
    TORCH_CHECK(has_cos == has_sin, "split_heads_rownorm: freqs_cos and freqs_sin come together");
    TORCH_CHECK(rope_mask == 0 || has_cos, "split_heads_rownorm: a rotated part needs freqs_cos / freqs_sin");
    if (has_cos) {
        fcc = freqs_cos->contiguous(), fsc = freqs_sin->contiguous();
        CHECK_DEV(fcc); CHECK_DEV(fsc);
        TORCH_CHECK(fcc.scalar_type() == at::kFloat && fsc.scalar_type() == at::kFloat && fcc.dim() == 2 && fcc.size(1) == 128 &&
                    fsc.sizes() == fcc.sizes() && fcc.size(0) <= n, "split_heads_rownorm: freqs must be float32 [rows <= n, 128]");
        fc = fcc.data_ptr<float>(), fs = fsc.data_ptr<float>(), rope_rows = fcc.size(0);
    }
    c10::DeviceGuard guard(x.device());
    at::Tensor out = at::empty({parts, B, heads, n, 128}, x.options());
    void *op[3] = {nullptr, nullptr, nullptr};
    std::vector<at::Tensor> res;
    for (int p = 0; p < parts; ++p) res.push_back(out[p]), op[p] = res.back().data_ptr();
    if (n == 0) return res;
    check(chipmunk_split_heads_rownorm(x.data_ptr(), x.dim() == 3 ? x.stride(0) : 0, x.stride(-2), (int)parts, wp[0], wd[0], wp[1], wd[1], wp[2],
                                       wd[2], op[0], op[1], op[2], (unsigned)norm_mask, (unsigned)rope_mask, B, n, (int)heads, (float)eps, fc,
                                       fs, rope_rows, cur_stream(x)),
          "split_heads_rownorm");
    return res;
}

// dst[..., i, :] = src[..., map[i], :] over the second-to-last axis (token reorder; see chipmunk_gather_rows)
at::Tensor gather_rows(at::Tensor src, at::Tensor map) {
    CHECK_DEV(src);
    CHECK_DEV(map);
    TORCH_CHECK(src.dim() >= 2, "gather_rows: src must be [..., n, d]");
    TORCH_CHECK(map.scalar_type() == at::kInt && map.dim() == 1 && map.is_contiguous(), "gather_rows: map must be a contiguous int32 vector");
    src = src.contiguous();
    const int64_t n_src = src.size(-2), d = src.size(-1), n_out = map.numel();
    const int64_t outer = n_src * d == 0 ? 0 : src.numel() / (n_src * d);
    auto sizes = src.sizes().vec();
    sizes[sizes.size() - 2] = n_out;
    c10::DeviceGuard guard(src.device());
    at::Tensor dst = at::empty(sizes, src.options());
    if (dst.numel() == 0) return dst;
    check(chipmunk_gather_rows(src.data_ptr(), dst.data_ptr(), map.data_ptr<int>(), outer, n_src, n_out,
                               d * (int64_t)src.element_size(), cur_stream(src)),
          "gather_rows");
    return dst;
}

}  // namespace

// schemas: byte-identical to reference csrc/chipmunk.cpp:47-60 (including its un-annotated mutations of `o`,
// `mma_c` and `counts`), followed by this build's additions.
TORCH_LIBRARY(chipmunk, m) {
    m.def("csp_mlp_mm1(Tensor a, Tensor b_colmajor, Tensor(c!) c, Tensor bias, Tensor pa_cache_colmajor, Tensor indices, Tensor indices_counts) -> ()");
    m.def("csp_mlp_mm2_and_scatter_add(Tensor packed, Tensor(unpacked_colmajor!) unpacked_colmajor, Tensor sp_inds, Tensor sp_counts, Tensor mma_a, Tensor mma_b, Tensor mma_c, int num_sms_scatter_add, int matmul_kernel) -> ()");

    m.def("csp_attn(Tensor q, Tensor k, Tensor v, Tensor o, Tensor indices, Tensor indices_counts, int o_scale) -> ()");
    m.def("csp_128_attn(Tensor q, Tensor k, Tensor v, Tensor indices, Tensor indices_counts) -> Tensor");
    m.def("dense_attn(Tensor q, Tensor k, Tensor v) -> Tensor[]");
    m.def("dense_colsum_attn(Tensor q, Tensor k, Tensor v, Tensor p) -> Tensor[]");

    m.def("copy_indices(Tensor bmfc1, Tensor(bm_mid_cache!) bm_mid_cache, Tensor sp_inds, Tensor sp_counts) -> ()");
    m.def("topk_indices(Tensor activation, Tensor(indices!) indices, Tensor counts, float sparsity_amount, int multiple_of, float random_amount) -> ()");
    m.def("csp_scatter_add(Tensor packed, Tensor(unpacked_colmajor!) unpacked_colmajor, Tensor sp_inds, Tensor sp_counts, int num_sms) -> ()");
    m.def("mask_to_indices(Tensor mask, int multiple_of, int pad_to_multiple_of) -> Tensor[]");

    // additions (not in the reference): native GEMM2 entry, fused packed-mask path, single-kernel bit packing
    m.def("csp_attn_out(Tensor q, Tensor k, Tensor v, Tensor o_in, Tensor indices, Tensor indices_counts, int o_scale) -> Tensor");
    m.def("csp_mlp_mm1_scatter(Tensor a, Tensor b_colmajor, Tensor(c!) c, Tensor bias, Tensor(pa_cache_colmajor!) pa_cache_colmajor, Tensor indices, Tensor indices_counts) -> ()");
    m.def("csp_mlp_mm2(Tensor mma_a, Tensor mma_b, Tensor indices, Tensor counts, Tensor(mma_c!) mma_c) -> ()");
    m.def("csp_mlp_mm2_w8(Tensor mma_a, Tensor mma_b, Tensor scale_b, Tensor indices, Tensor counts, Tensor(mma_c!) mma_c) -> ()");
    m.def("csp_mlp_mm1_fp8(Tensor a, Tensor b, Tensor(c!) c, Tensor bias, Tensor(pa_cache_colmajor!) pa_cache_colmajor, Tensor indices, Tensor indices_counts, Tensor scale_a, Tensor scale_b, bool update_cache) -> ()");
    m.def("csp_mlp_mm1_fp8_scatter(Tensor a, Tensor b, Tensor(c!) c, Tensor bias, Tensor(pa_cache_colmajor!) pa_cache_colmajor, Tensor indices, Tensor indices_counts, Tensor scale_a, Tensor scale_b) -> ()");
    m.def("csp_mlp_mm1_glu(Tensor a, Tensor b_gate, Tensor b_up, Tensor(c!) c, Tensor? bias_gate, Tensor? bias_up, Tensor(pa_cache_colmajor!) pa_cache_colmajor, Tensor indices, Tensor indices_counts, str act, bool update_cache) -> ()");
    m.def("csp_mlp_mm1_glu_fp8(Tensor a, Tensor b_gate, Tensor b_up, Tensor(c!) c, Tensor? bias_gate, Tensor? bias_up, Tensor(pa_cache_colmajor!) pa_cache_colmajor, Tensor indices, Tensor indices_counts, Tensor scale_a, Tensor scale_b_gate, Tensor scale_b_up, str act, bool update_cache) -> ()");
    m.def("csp_mlp_mm1_act(Tensor a, Tensor b, Tensor(c!) c, Tensor? bias, Tensor(pa!) pa_cache, Tensor indices, Tensor counts, str act, bool update_cache) -> ()");
    m.def("csp_mlp_mm1_w8(Tensor a, Tensor b, Tensor scale_b, Tensor(c!) c, Tensor? bias, Tensor(pa!) pa_cache, Tensor indices, Tensor counts, str act, bool update_cache) -> ()");
    m.def("csp_mlp_mm1_glu_w8(Tensor a, Tensor b_gate, Tensor b_up, Tensor scale_gate, Tensor scale_up, Tensor(c!) c, Tensor? bias_gate, Tensor? bias_up, Tensor(pa!) pa_cache, Tensor indices, Tensor counts, str act, bool update_cache) -> ()");
    m.def("w8_linear(Tensor x, Tensor w, Tensor scale_b, Tensor? bias, Tensor(a!) y) -> ()");
    m.def("csp_mlp_mm1_fp8_act(Tensor a, Tensor b, Tensor(c!) c, Tensor? bias, Tensor(pa!) pa_cache, Tensor indices, Tensor counts, Tensor scale_a, Tensor scale_b, str act, int update_cache) -> ()");
    m.def("topk_delta_indices(Tensor activation, Tensor(cache!) cache, Tensor(indices!) indices, Tensor(counts!) counts, float sparsity_amount, int multiple_of, float random_amount) -> ()");
    m.def("topk_indices_p(Tensor activation, Tensor(indices!) indices, Tensor(counts!) counts, float sparsity_amount, float top_p, float min_keys, int multiple_of, float random_amount) -> ()");
    m.def("topk_delta_indices_p(Tensor activation, Tensor(cache!) cache, Tensor(indices!) indices, Tensor(counts!) counts, float sparsity_amount, float top_p, float min_keys, int multiple_of, float random_amount) -> ()");
    m.def("topk_group_delta_indices(Tensor activation, Tensor(cache!) cache, Tensor(indices!) indices, Tensor(counts!) counts, int rows_per_group, float sparsity_amount, int multiple_of, float random_amount) -> ()");
    m.def("topk_group_delta_indices_p(Tensor activation, Tensor(cache!) cache, Tensor(indices!) indices, Tensor(counts!) counts, int rows_per_group, float sparsity_amount, float top_p, float min_keys, int multiple_of, float random_amount) -> ()");
    m.def("packed_mask_to_indices(Tensor packed, int[] shape, int multiple_of, int pad_to_multiple_of) -> Tensor[]");
    m.def("mask_to_sorted_indices(Tensor mask, int[] shape, int multiple_of, int pad_to_multiple_of) -> Tensor[]");
    m.def("topk_mask(Tensor cs, int k, float random_amount, Tensor? groups, Tensor? static_mask) -> Tensor");
    m.def("dense_colsum_topk_mask(Tensor q, Tensor k, Tensor v, Tensor p, int k_top, float random_amount, Tensor? groups, Tensor? static_mask, bool token_major_o=False) -> Tensor[]");
    m.def("topk_mask_p(Tensor cs, int k, float top_p, int k_min, float random_amount, Tensor? groups, Tensor? static_mask) -> Tensor");
    m.def("dense_colsum_topk_mask_p(Tensor q, Tensor k, Tensor v, Tensor p, int k_top, float top_p, int k_min, float random_amount, Tensor? groups, Tensor? static_mask, bool token_major_o=False) -> Tensor[]");
    // the two dense operators with a choice of output layout (the reference's schemas above stay as they are)
    m.def("dense_attn_layout(Tensor q, Tensor k, Tensor v, bool token_major_o) -> Tensor[]");
    m.def("dense_colsum_attn_layout(Tensor q, Tensor k, Tensor v, Tensor p, bool token_major_o) -> Tensor[]");
    // padded batches: the dense and mask-step operators with per-sequence key lengths, int32 [B] on the GPU
    m.def("dense_attn_varlen(Tensor q, Tensor k, Tensor v, Tensor k_lens, bool token_major_o=False) -> Tensor[]");
    m.def("dense_colsum_attn_varlen(Tensor q, Tensor k, Tensor v, Tensor p, Tensor k_lens, bool token_major_o=False) -> Tensor[]");
    m.def("topk_mask_varlen(Tensor cs, Tensor k_lens, int k, float random_amount, Tensor? groups, Tensor? static_mask) -> Tensor");
    m.def("topk_mask_p_varlen(Tensor cs, Tensor k_lens, int k, float top_p, int k_min, float random_amount, Tensor? groups, Tensor? static_mask) -> Tensor");
    m.def("dense_colsum_topk_mask_varlen(Tensor q, Tensor k, Tensor v, Tensor p, Tensor k_lens, int k_top, float random_amount, Tensor? groups, Tensor? static_mask, bool token_major_o=False) -> Tensor[]");
    m.def("dense_colsum_topk_mask_p_varlen(Tensor q, Tensor k, Tensor v, Tensor p, Tensor k_lens, int k_top, float top_p, int k_min, float random_amount, Tensor? groups, Tensor? static_mask, bool token_major_o=False) -> Tensor[]");
    m.def("compact_indices(Tensor indices, Tensor counts) -> Tensor[]");
    m.def("mask_to_ragged_indices(Tensor mask, int[] shape, int multiple_of, int pad_to_multiple_of, bool sorted) -> Tensor[]");
    m.def("csp_attn_out_ragged(Tensor q, Tensor k, Tensor v, Tensor o_in, Tensor indices, Tensor offsets, Tensor indices_counts, int o_scale) -> Tensor");
    m.def("residual_ln_modulate(Tensor x, Tensor? y, Tensor? gate, Tensor shift, Tensor scale, float eps) -> Tensor[]");
    m.def("residual_ln_modulate_f32(Tensor x, Tensor? y, Tensor? gate, Tensor? shift, Tensor? scale, Tensor? weight, Tensor? bias, float eps) -> Tensor[]");
    m.def("transpose_last2(Tensor x) -> Tensor");
    m.def("transpose_last2_pitched(Tensor x, int ld) -> Tensor");
    m.def("transpose_to_groups(Tensor x) -> Tensor");
    m.def("csp_scatter_add_gm(Tensor packed, Tensor(unpacked_groups!) unpacked_groups, Tensor sp_inds, Tensor sp_counts) -> ()");
    m.def("block_mean(Tensor x, int mbm) -> Tensor");
    m.def("quantize_fp8(Tensor x, Tensor scale, float max_value) -> Tensor");
    m.def("quantize_fp8_rowwise(Tensor x, float max_value) -> Tensor[]");
    m.def("csp_mlp_mm1_fp8_act_rs(Tensor a, Tensor b, Tensor(c!) c, Tensor? bias, Tensor(pa!) pa_cache, Tensor indices, Tensor counts, Tensor scale_a, Tensor scale_b, str act, int update_cache) -> ()");
    m.def("bitpack(Tensor mask) -> Tensor");
    m.def("bitunpack(Tensor packed, int[] shape) -> Tensor");
    m.def("gather_rows(Tensor src, Tensor map) -> Tensor");
    m.def("qkv_split_norm(Tensor qkv, Tensor? q_weight, Tensor? k_weight, int heads, float eps, Tensor? freqs_cos=None, Tensor? freqs_sin=None) -> Tensor[]");
    m.def("split_heads_rownorm(Tensor x, int heads, int parts, Tensor? w0, Tensor? w1, Tensor? w2, int norm_mask, int rope_mask, float eps, Tensor? freqs_cos=None, Tensor? freqs_sin=None) -> Tensor[]");
}

TORCH_LIBRARY_IMPL(chipmunk, CUDA, m) {
    m.impl("qkv_split_norm", &qkv_split_norm);
    m.impl("split_heads_rownorm", &split_heads_rownorm);
    m.impl("csp_mlp_mm1_fp8_scatter", &csp_mlp_mm1_fp8_scatter);
    m.impl("dense_colsum_topk_mask", &dense_colsum_topk_mask);
    m.impl("dense_colsum_topk_mask_p", &dense_colsum_topk_mask_p);
    m.impl("csp_mlp_mm1", &csp_mlp_mm1);
    m.impl("csp_mlp_mm2_and_scatter_add", &csp_mlp_mm2_and_scatter_add);
    m.impl("copy_indices", &copy_indices);
    m.impl("topk_indices", &topk_indices);
    m.impl("csp_scatter_add", &csp_scatter_add);
    m.impl("mask_to_indices", &mask_to_indices);
    m.impl("csp_attn", &csp_attn);
    m.impl("csp_128_attn", &csp_128_attn);
    m.impl("dense_attn", &dense_attn);
    m.impl("dense_colsum_attn", &dense_colsum_attn);
    m.impl("compact_indices", &compact_indices);
    m.impl("residual_ln_modulate", &residual_ln_modulate);
    m.impl("residual_ln_modulate_f32", &residual_ln_modulate_f32);
    m.impl("csp_attn_out_ragged", &csp_attn_out_ragged);
    m.impl("dense_attn_varlen", &dense_attn_varlen);
    m.impl("dense_colsum_attn_varlen", &dense_colsum_attn_varlen);
    m.impl("topk_mask_varlen", &topk_mask_varlen);
    m.impl("topk_mask_p_varlen", &topk_mask_p_varlen);
    m.impl("dense_colsum_topk_mask_varlen", &dense_colsum_topk_mask_varlen);
    m.impl("dense_colsum_topk_mask_p_varlen", &dense_colsum_topk_mask_p_varlen);
    m.impl("dense_attn_layout", &dense_attn_layout);
    m.impl("dense_colsum_attn_layout", &dense_colsum_attn_layout);
    m.impl("csp_attn_out", &csp_attn_out);
    m.impl("csp_mlp_mm1_scatter", &csp_mlp_mm1_scatter);
    m.impl("csp_mlp_mm2", &csp_mlp_mm2);
    m.impl("csp_mlp_mm2_w8", &csp_mlp_mm2_w8);
    m.impl("csp_mlp_mm1_fp8", &csp_mlp_mm1_fp8);
    m.impl("csp_mlp_mm1_glu", &csp_mlp_mm1_glu);
    m.impl("csp_mlp_mm1_glu_fp8", &csp_mlp_mm1_glu_fp8);
    m.impl("csp_mlp_mm1_act", &csp_mlp_mm1_act);
    m.impl("csp_mlp_mm1_w8", &csp_mlp_mm1_w8);
    m.impl("csp_mlp_mm1_glu_w8", &csp_mlp_mm1_glu_w8);
    m.impl("w8_linear", &w8_linear);
    m.impl("csp_mlp_mm1_fp8_act", &csp_mlp_mm1_fp8_act);
    m.impl("topk_delta_indices", &topk_delta_indices);
    m.impl("topk_indices_p", &topk_indices_p);
    m.impl("topk_delta_indices_p", &topk_delta_indices_p);
    m.impl("topk_group_delta_indices", &topk_group_delta_indices);
    m.impl("topk_group_delta_indices_p", &topk_group_delta_indices_p);
    m.impl("packed_mask_to_indices", &packed_mask_to_indices);
    m.impl("mask_to_sorted_indices", &mask_to_sorted_indices);
    m.impl("mask_to_ragged_indices", &mask_to_ragged_indices);
    m.impl("topk_mask", &topk_mask);
    m.impl("topk_mask_p", &topk_mask_p);
    m.impl("transpose_last2", &transpose_last2);
    m.impl("transpose_last2_pitched", &transpose_last2_pitched);
    m.impl("transpose_to_groups", &transpose_to_groups);
    m.impl("csp_scatter_add_gm", &csp_scatter_add_gm);
    m.impl("block_mean", &block_mean);
    m.impl("quantize_fp8", &quantize_fp8);
    m.impl("quantize_fp8_rowwise", &quantize_fp8_rowwise);
    m.impl("csp_mlp_mm1_fp8_act_rs", &csp_mlp_mm1_fp8_act_rs);
    m.impl("bitpack", &bitpack);
    m.impl("bitunpack", &bitunpack);
    m.impl("gather_rows", &gather_rows);
}

}  // namespace chipmunk
