// PyTorch-ROCm custom-op layer of fabhip: TORCH_LIBRARY(fabhip, ...) over the C ABI of libfabhip.so
// (include/fabhip.h).  This is how the Python mirror of fab-torch's plug-in interfaces reaches the HIP kernels
// (north_star: "called from Python through PyTorch-ROCm custom ops"; SURVEY.md section 8b, "Torch op layer").
//
//  * every op is registered for the CUDA (= HIP on ROCm) dispatch key ONLY: there is no CPU kernel, a CPU tensor
//    fails in the dispatcher ("could not run fabhip::... with arguments from the 'CPU' backend");
//  * ops only translate tensors into the raw-pointer argument structs of the C ABI, allocate outputs / scratch
//    through torch's caching allocator (stream-ordered, so scratch is never shared between streams) and enqueue on
//    the current HIP stream; no synchronisation, no host reads;
//  * a non-zero fabhip return code becomes a c10::Error (Python RuntimeError) via TORCH_CHECK;
//  * autograd for the training op (fabhip::realnvp_logprob_tape) is registered from Python with
//    torch.library.register_autograd (fab_torch_amd/_ops.py); its backward is fabhip::realnvp_param_grad.
//
// Flow parameters travel as `Tensor[] params` in the order of fabhip_flow_params: per layer
// {w1, b1, w2, b2, w3, b3, L, U, log_S, sign_S, P}, then {loc, log_scale}, then (act_norm flows only) one
// {ActNorm.s, ActNorm.t} pair per layer.  Targets travel as
// (int kind, float[] {a, b, c, log_norm}, Tensor? locs, Tensor? scales).
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>
#include <torch/csrc/distributed/c10d/GroupRegistry.hpp>
#include <torch/csrc/distributed/c10d/ProcessGroup.hpp>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fabhip.h"

namespace {

using at::Tensor;
using c10::optional;

fabhip_stream_t stream_of(const Tensor& t) {
    return (fabhip_stream_t)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.get_device()).stream();
}

void chk(int rc, const char* what) {
    TORCH_CHECK(rc == FABHIP_OK, "fabhip ", what, " failed: ", fabhip_strerror(rc), " (code ", rc, ")");
}

void need(const Tensor& t, at::ScalarType st, const char* name) {
    TORCH_CHECK(t.is_cuda(), "fabhip: ", name, " must live on the GPU (no CPU path)");
    TORCH_CHECK(t.scalar_type() == st, "fabhip: ", name, " has dtype ", t.scalar_type(), ", expected ", st);
    TORCH_CHECK(t.is_contiguous(), "fabhip: ", name, " must be contiguous");
}
const float* fp(const Tensor& t, const char* name) { need(t, at::kFloat, name); return t.data_ptr<float>(); }
float* fpm(const Tensor& t, const char* name) { need(t, at::kFloat, name); return t.data_ptr<float>(); }
float* fpm_opt(const optional<Tensor>& t, const char* name) { return t.has_value() ? fpm(*t, name) : nullptr; }
const float* fp_opt(const optional<Tensor>& t, const char* name) { return t.has_value() ? fp(*t, name) : nullptr; }

// The kernels index raw pointers: every tensor whose pointer goes into an argument struct is checked for its element
// count and for living on the device of the tensor the launch is enqueued for (`ref`).  `at_least`: n is a lower bound.
void need_n(const Tensor& t, int64_t n, const Tensor& ref, const char* name, bool at_least = false) {
    TORCH_CHECK(t.device() == ref.device(), "fabhip: ", name, " is on ", t.device(), ", expected ", ref.device());
    TORCH_CHECK(at_least ? t.numel() >= n : t.numel() == n, "fabhip: ", name, " has ", t.numel(), " elements, expected ",
                at_least ? "at least " : "", n);
}
const float* fpn(const Tensor& t, int64_t n, const Tensor& ref, const char* name) { need_n(t, n, ref, name); return fp(t, name); }
float* fpmn(const Tensor& t, int64_t n, const Tensor& ref, const char* name, bool at_least = false) {
    need_n(t, n, ref, name, at_least);
    return fpm(t, name);
}
float* fpmn_opt(const optional<Tensor>& t, int64_t n, const Tensor& ref, const char* name, bool at_least = false) {
    return t.has_value() ? fpmn(*t, n, ref, name, at_least) : nullptr;
}

Tensor fempty(at::IntArrayRef shape, const Tensor& like) { return at::empty(shape, like.options().dtype(at::kFloat)); }
Tensor scratch(size_t bytes, const Tensor& like) {
    return at::empty({(int64_t)(bytes + 256)}, like.options().dtype(at::kByte));
}
void* aligned(const Tensor& ws) {
    auto p = (uintptr_t)ws.data_ptr();
    return (void*)((p + 255) & ~(uintptr_t)255);
}

fabhip_flow make_flow(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t precision = 0) {
    fabhip_flow f;
    TORCH_CHECK(precision >= 0 && precision <= 2, "fabhip: precision must be 0 (process default), 1 (fp32) or 2 (fast)");
    f.dim = (int32_t)dim; f.n_layers = (int32_t)n_layers; f.width = (int32_t)width; f.precision = (int32_t)precision;
    f.packed = fp(packed, "packed flow image");
    const int64_t n = fabhip_flow_packed_floats(f.dim, f.n_layers, f.width);
    TORCH_CHECK(n > 0, "fabhip: flow shape not supported (dim ", dim, ", width ", width, ")");
    TORCH_CHECK(packed.numel() == n, "fabhip: packed image has ", packed.numel(), " floats, expected ", n);
    return f;
}

void fill_params(fabhip_flow_params& p, at::TensorList params, int64_t dim, int64_t n_layers, int64_t width) {
    TORCH_CHECK(n_layers >= 1 && n_layers <= FABHIP_MAX_LAYERS, "fabhip: n_layers out of range");
    const bool act_norm = (int64_t)params.size() == 13 * n_layers + 2;
    TORCH_CHECK(act_norm || (int64_t)params.size() == 11 * n_layers + 2, "fabhip: expected ", 11 * n_layers + 2,
                " parameter tensors (11 per layer + loc + log_scale), or ", 13 * n_layers + 2,
                " with one ActNorm {s, t} pair per layer appended, got ", params.size());
    p.dim = (int32_t)dim; p.n_layers = (int32_t)n_layers; p.width = (int32_t)width;
    const int64_t d = (dim + 1) / 2, DO = dim - d;     // make_normflow_model.py:17 `int(dim / 2 + 0.5)`
    const int64_t want[11] = {width * d, width, width * width, width, 2 * DO * width, 2 * DO, dim * dim, dim * dim, dim, dim,
                              dim * dim};
    static const char* names[11] = {"w1", "b1", "w2", "b2", "w3", "b3", "L", "U", "log_S", "sign_S", "P"};
    for (int64_t k = 0; k < n_layers; ++k) {
        const Tensor* t = &params[11 * k];
        for (int i = 0; i < 11; ++i) need_n(t[i], want[i], params[0], names[i]);
        p.w1[k] = fp(t[0], "w1"); p.b1[k] = fp(t[1], "b1"); p.w2[k] = fp(t[2], "w2"); p.b2[k] = fp(t[3], "b2");
        p.w3[k] = fp(t[4], "w3"); p.b3[k] = fp(t[5], "b3"); p.lu_L[k] = fp(t[6], "L"); p.lu_U[k] = fp(t[7], "U");
        p.log_S[k] = fp(t[8], "log_S"); p.sign_S[k] = fp(t[9], "sign_S"); p.perm_P[k] = fp(t[10], "P");
    }
    p.loc = fpn(params[11 * n_layers], dim, params[0], "loc");
    p.log_scale = fpn(params[11 * n_layers + 1], dim, params[0], "log_scale");
    for (int64_t k = 0; k < FABHIP_MAX_LAYERS; ++k) { p.an_s[k] = nullptr; p.an_t[k] = nullptr; }
    if (act_norm)
        for (int64_t k = 0; k < n_layers; ++k) {
            const Tensor &s = params[11 * n_layers + 2 + 2 * k], &t = params[11 * n_layers + 3 + 2 * k];
            need_n(s, dim, params[0], "ActNorm.s"); need_n(t, dim, params[0], "ActNorm.t");
            p.an_s[k] = fp(s, "ActNorm.s"); p.an_t[k] = fp(t, "ActNorm.t");
        }
}

// `ref`: the tensor whose device the launch is enqueued for (the quartic and the rotor target's tensors must live there).
fabhip_target make_target(int64_t kind, at::ArrayRef<double> prm, const optional<Tensor>& locs,
                          const optional<Tensor>& scales, int64_t dim, const Tensor& ref) {
    TORCH_CHECK(prm.size() == 4, "fabhip: target parameters are {a, b, c, log_norm}");
    fabhip_target t;
    t.kind = (int32_t)kind; t.dim = (int32_t)dim;
    t.a = (float)prm[0]; t.b = (float)prm[1]; t.c = (float)prm[2]; t.log_norm = (float)prm[3];
    t.n_mix = 0; t.locs = nullptr; t.scales = nullptr;
    if (kind == FABHIP_TARGET_GMM) {
        TORCH_CHECK(locs.has_value() && scales.has_value(), "fabhip: GMM target needs locs and scales");
        t.locs = fp(*locs, "locs"); t.scales = fp(*scales, "scales");
        t.n_mix = (int32_t)locs->size(0);
        TORCH_CHECK(locs->dim() == 2 && locs->size(1) == dim && scales->sizes() == locs->sizes(), "fabhip: GMM shapes");
    }
    if (kind == FABHIP_TARGET_QUARTIC) {      // locs = coupling J [D, D] (symmetric), scales = site coefficients [3, D]
        TORCH_CHECK(locs.has_value() && scales.has_value(), "fabhip: quartic target needs the coupling (locs) and the site "
                    "coefficients (scales)");
        TORCH_CHECK(dim >= 1 && dim <= FABHIP_MAX_DIM, "fabhip: quartic target needs 1 <= dim <= ", FABHIP_MAX_DIM, ", got ", dim);
        TORCH_CHECK(locs->dim() == 2 && locs->size(0) == dim && locs->size(1) == dim, "fabhip: quartic coupling must be [",
                    dim, ", ", dim, "], got ", locs->sizes());
        TORCH_CHECK(scales->dim() == 2 && scales->size(0) == 3 && scales->size(1) == dim, "fabhip: quartic site coefficients "
                    "must be [3, ", dim, "], got ", scales->sizes());
        t.locs = fpn(*locs, dim * dim, ref, "quartic coupling"); t.scales = fpn(*scales, 3 * dim, ref, "quartic site coefficients");
    }
    if (kind == FABHIP_TARGET_ROTOR) {        // locs = neighbour table [2 NB, D] (indices, then couplings), scales = site rows [9, D]
        TORCH_CHECK(locs.has_value() && scales.has_value(), "fabhip: rotor target needs the neighbour table (locs) and the site "
                    "rows (scales)");
        TORCH_CHECK(dim >= 1 && dim <= FABHIP_MAX_DIM, "fabhip: rotor target needs 1 <= dim <= ", FABHIP_MAX_DIM, ", got ", dim);
        TORCH_CHECK(scales->dim() == 2 && scales->size(0) == 9 && scales->size(1) == dim, "fabhip: rotor site rows must be [9, ",
                    dim, "], got ", scales->sizes());
        TORCH_CHECK(locs->dim() == 2 && locs->size(1) == dim && locs->size(0) % 2 == 0, "fabhip: rotor neighbour table must be "
                    "[2 NB, ", dim, "], got ", locs->sizes());
        const int64_t nb = locs->size(0) / 2;
        TORCH_CHECK(nb >= 1 && nb <= FABHIP_MAX_DIM - 1, "fabhip: rotor neighbour table needs 1 <= NB <= ", FABHIP_MAX_DIM - 1,
                    ", got ", nb);
        t.n_mix = (int32_t)nb;
        t.locs = fpn(*locs, 2 * nb * dim, ref, "rotor neighbour table"); t.scales = fpn(*scales, 9 * dim, ref, "rotor site rows");
    }
    return t;
}

fabhip_anneal coefs(double beta, double alpha, bool p_target) {
    fabhip_anneal a;
    fabhip_anneal_coefs(beta, alpha, p_target ? 1 : 0, &a);
    return a;
}

// ------------------------------------------------------------------------------------------------------------------
// geometry queries (no tensors: catch-all kernels)
// ------------------------------------------------------------------------------------------------------------------
int64_t abi_version() { return fabhip_version(); }
int64_t flow_packed_floats(int64_t dim, int64_t n_layers, int64_t width) {
    return fabhip_flow_packed_floats((int32_t)dim, (int32_t)n_layers, (int32_t)width);
}
// Identity of a parameter set: two independent 64-bit mixes over (storage address, version counter) of every tensor, in
// order - what flow.native() compares to decide whether the packed image is current.  One call instead of two Python
// attribute reads per tensor (112 tensors for the headline flow: 90 us of host time per AIS call, during which the GPU idles).
std::vector<int64_t> tensors_key(at::TensorList ts) {
    uint64_t h1 = 0x9E3779B97F4A7C15ull, h2 = 0xC2B2AE3D27D4EB4Full;
    auto mix = [](uint64_t h, uint64_t v, uint64_t m) {
        h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
        h *= m;
        return h ^ (h >> 29);
    };
    for (const Tensor& t : ts) {
        const uint64_t p = t.defined() ? (uint64_t)(uintptr_t)t.data_ptr() : 0, v = t.defined() ? (uint64_t)t._version() : 0;
        h1 = mix(mix(h1, p, 0xBF58476D1CE4E5B9ull), v, 0x94D049BB133111EBull);
        h2 = mix(mix(h2, v ^ 0x5555555555555555ull, 0xD6E8FEB86659FD93ull), p, 0xFF51AFD7ED558CCDull);
    }
    return {(int64_t)h1, (int64_t)h2, (int64_t)ts.size()};
}
// The same for a parameter set registered once: the op layer keeps the tensor handles (the Python side keeps the objects alive
// and re-registers when the set itself changes), so the per-call check passes ONE integer through the dispatcher instead of a
// list of 112 tensors.  `param.data = ...`, `.to()`, load_state_dict and in-place updates all act on the registered TensorImpl.
static std::mutex g_keysets_mu;
static std::vector<std::vector<Tensor>> g_keysets;
static std::vector<int64_t> g_keysets_free;        // released slots (tensors_key_release)
int64_t tensors_key_register(at::TensorList ts, int64_t reuse) {
    std::lock_guard<std::mutex> lk(g_keysets_mu);
    std::vector<Tensor> v(ts.begin(), ts.end());
    // (a slot is re-used only while its owner still holds it: one that has been released - and may have been handed to another
    //  flow since - is not the caller's any more)
    if (reuse >= 0 && reuse < (int64_t)g_keysets.size() &&
        std::find(g_keysets_free.begin(), g_keysets_free.end(), reuse) == g_keysets_free.end()) {
        g_keysets[(size_t)reuse] = std::move(v);
        return reuse;
    }
    if (!g_keysets_free.empty()) {
        const int64_t h = g_keysets_free.back();
        g_keysets_free.pop_back();
        g_keysets[(size_t)h] = std::move(v);
        return h;
    }
    g_keysets.push_back(std::move(v));
    return (int64_t)g_keysets.size() - 1;
}
// a flow that is garbage-collected gives its slot back (the handles of dropped tensors are released; the slot is reused)
void tensors_key_release(int64_t handle) {
    std::lock_guard<std::mutex> lk(g_keysets_mu);
    if (handle < 0 || handle >= (int64_t)g_keysets.size()) return;
    if (std::find(g_keysets_free.begin(), g_keysets_free.end(), handle) != g_keysets_free.end()) return;   // already free: a second
                                                                                       // release must not hand the slot out twice
    g_keysets[(size_t)handle].clear();
    g_keysets[(size_t)handle].shrink_to_fit();
    g_keysets_free.push_back(handle);
}
std::vector<int64_t> tensors_key_of(int64_t handle) {
    std::lock_guard<std::mutex> lk(g_keysets_mu);
    TORCH_CHECK(handle >= 0 && handle < (int64_t)g_keysets.size(), "fabhip: unknown parameter-set handle ", handle);
    return tensors_key(g_keysets[(size_t)handle]);
}
int64_t flow_grad_floats(int64_t dim, int64_t n_layers, int64_t width) {
    return fabhip_flow_grad_floats((int32_t)dim, (int32_t)n_layers, (int32_t)width);
}
std::vector<int64_t> flow_grad_layout(int64_t dim, int64_t n_layers, int64_t width) {
    std::vector<int64_t> out(15);
    chk(fabhip_flow_grad_layout((int32_t)dim, (int32_t)n_layers, (int32_t)width, out.data()), "flow_grad_layout");
    return out;
}
int64_t set_fast_mode(bool on) { return fabhip_set_fast_mode(on ? 1 : 0); }
int64_t get_fast_mode() { return fabhip_get_fast_mode(); }
int64_t set_option(int64_t key, int64_t value) {
    const int prev = fabhip_set_option((int)key, (int)value);
    TORCH_CHECK(!(prev < 0 && (key < 0 || key >= FABHIP_OPT_COUNT)), "fabhip: unknown option key ", key);
    return prev;
}
int64_t get_option(int64_t key) {
    TORCH_CHECK(key >= 0 && key < FABHIP_OPT_COUNT, "fabhip: unknown option key ", key);
    return fabhip_get_option((int)key);
}
std::vector<int64_t> flow_tape_layout(int64_t dim, int64_t n_layers, int64_t width, int64_t B) {
    std::vector<int64_t> out(18);
    chk(fabhip_flow_tape_layout((int32_t)dim, (int32_t)n_layers, (int32_t)width, B, out.data()), "flow_tape_layout");
    return out;
}
int64_t spline_packed_floats(int64_t dim, int64_t n_layers, int64_t hidden) {
    return fabhip_spline_packed_floats((int32_t)dim, (int32_t)n_layers, (int32_t)hidden);
}
std::vector<double> anneal_coefs(double beta, double alpha, bool p_target) {
    const fabhip_anneal a = coefs(beta, alpha, p_target);
    return {a.c_q, a.c_p, a.g_q, a.g_p};
}

// ------------------------------------------------------------------------------------------------------------------
// RealNVP flow
// ------------------------------------------------------------------------------------------------------------------
void realnvp_pack(at::TensorList params, int64_t dim, int64_t n_layers, int64_t width, bool with_inverse,
                  Tensor packed) {
    c10::DeviceGuard g(packed.device());
    fabhip_flow_params p;
    fill_params(p, params, dim, n_layers, width);
    make_flow(packed, dim, n_layers, width);
    auto fn = with_inverse ? fabhip_flow_pack : fabhip_flow_pack_density;
    chk(fn(&p, packed.data_ptr<float>(), stream_of(packed)), "flow_pack");
}

std::tuple<Tensor, Tensor> realnvp_sample(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width,
                                          const Tensor& eps) {
    c10::DeviceGuard g(eps.device());
    const fabhip_flow f = make_flow(packed, dim, n_layers, width);
    TORCH_CHECK(eps.dim() == 2 && eps.size(1) == dim, "fabhip: eps must be [B, dim]");
    const int64_t B = eps.size(0);
    Tensor x = at::empty_like(eps), log_q = fempty({B}, eps);
    chk(fabhip_flow_sample(&f, fp(eps, "eps"), x.data_ptr<float>(), log_q.data_ptr<float>(), B, stream_of(eps)),
        "flow_sample");
    return {x, log_q};
}

std::tuple<Tensor, Tensor> realnvp_logprob_grad(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width,
                                                const Tensor& x, bool with_grad, int64_t precision) {
    c10::DeviceGuard g(x.device());
    const fabhip_flow f = make_flow(packed, dim, n_layers, width, precision);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [B, dim]");
    const int64_t B = x.size(0);
    Tensor log_q = fempty({B}, x), grad = with_grad ? at::empty_like(x) : fempty({0}, x);
    chk(fabhip_flow_log_prob(&f, fp(x, "x"), log_q.data_ptr<float>(), with_grad ? grad.data_ptr<float>() : nullptr, B,
                             stream_of(x)),
        "flow_log_prob");
    return {log_q, grad};
}

// the differentiable training op: log q(x) with a tape; `theta` (the flat parameter image, or any tensor the
// parameters are a differentiable function of) is not read - it is the autograd handle of the parameters
std::tuple<Tensor, Tensor, Tensor> realnvp_logprob_tape(const Tensor& theta, const Tensor& x, const Tensor& packed,
                                                        at::TensorList params, int64_t dim, int64_t n_layers,
                                                        int64_t width, bool want_grad_x) {
    (void)theta; (void)params;
    c10::DeviceGuard g(x.device());
    const fabhip_flow f = make_flow(packed, dim, n_layers, width);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [B, dim]");
    const int64_t B = x.size(0);
    const size_t nbytes = fabhip_flow_tape_bytes(f.dim, f.n_layers, f.width, B);
    Tensor log_q = fempty({B}, x), grad = want_grad_x ? at::empty_like(x) : fempty({0}, x);
    Tensor tape = fempty({(int64_t)(nbytes / 4 + 1)}, x);
    chk(fabhip_flow_log_prob_tape(&f, fp(x, "x"), log_q.data_ptr<float>(),
                                  want_grad_x ? grad.data_ptr<float>() : nullptr, B, tape.data_ptr<float>(), nbytes,
                                  stream_of(x)),
        "flow_log_prob_tape");
    return {log_q, grad, tape};
}

Tensor realnvp_param_grad(at::TensorList params, const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width,
                          const Tensor& tape, const Tensor& coef) {
    c10::DeviceGuard g(coef.device());
    fabhip_flow_params p;
    fill_params(p, params, dim, n_layers, width);
    const fabhip_flow f = make_flow(packed, dim, n_layers, width);
    const int64_t B = coef.size(0);
    const size_t nbytes = fabhip_flow_tape_bytes(f.dim, f.n_layers, f.width, B);
    TORCH_CHECK((size_t)tape.numel() * 4 >= nbytes, "fabhip: tape too small for ", B, " rows");
    int64_t lay[15];
    chk(fabhip_flow_grad_layout(f.dim, f.n_layers, f.width, lay), "flow_grad_layout");
    Tensor flat = fempty({p.an_s[0] ? lay[14] : lay[12]}, coef);     // ActNorm flows: + [an_s | an_t] per layer
    chk(fabhip_flow_param_grad(&p, &f, fp(tape, "tape"), nbytes, fp(coef, "coef"), B, flat.data_ptr<float>(),
                               stream_of(coef)),
        "flow_param_grad");
    return flat;
}

// the differentiable sampling op (reparameterised baseline losses, fab/core.py:130-152): forward = fabhip_flow_sample;
// autograd is registered from Python (_ops.py), its backward = realnvp_sample_grad_tape + realnvp_param_grad(coef = 1).
// `theta` is the autograd handle of the parameters, as in realnvp_logprob_tape.
std::tuple<Tensor, Tensor> realnvp_sample_tape(const Tensor& theta, const Tensor& eps, const Tensor& packed,
                                               at::TensorList params, int64_t dim, int64_t n_layers, int64_t width) {
    (void)theta; (void)params;
    return realnvp_sample(packed, dim, n_layers, width, eps);
}

std::tuple<Tensor, Tensor> realnvp_sample_grad_tape(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width,
                                                    const Tensor& x, const Tensor& grad_x, const Tensor& grad_log_q) {
    c10::DeviceGuard g(x.device());
    const fabhip_flow f = make_flow(packed, dim, n_layers, width);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [B, dim]");
    const int64_t B = x.size(0);
    TORCH_CHECK(grad_x.dim() == 2 && grad_x.size(0) == B && grad_x.size(1) == dim && grad_log_q.numel() == B,
                "fabhip: grad_x must be [B, dim] and grad_log_q [B]");
    const size_t nbytes = fabhip_flow_tape_bytes(f.dim, f.n_layers, f.width, B);
    Tensor tape = fempty({(int64_t)(nbytes / 4 + 1)}, x), g_eps = at::empty_like(x);
    chk(fabhip_flow_sample_grad_tape(&f, fp(x, "x"), fp(grad_x, "grad_x"), fp(grad_log_q, "grad_log_q"),
                                     g_eps.data_ptr<float>(), B, tape.data_ptr<float>(), nbytes, stream_of(x)),
        "flow_sample_grad_tape");
    return {tape, g_eps};
}

void adam_clip_step(Tensor theta, const Tensor& grad, Tensor m, Tensor v, double lr, double beta1, double beta2,
                    double eps, Tensor step_count, double max_norm, Tensor grad_norm) {
    c10::DeviceGuard g(theta.device());
    const int64_t n = theta.numel();
    TORCH_CHECK(grad.numel() == n && m.numel() == n && v.numel() == n, "fabhip: adam image sizes differ");
    need(step_count, at::kInt, "step_count");
    const size_t nb = fabhip_adam_workspace_bytes(n);
    Tensor ws = scratch(nb, theta);
    chk(fabhip_adam_clip_step(fpm(theta, "theta"), fp(grad, "grad"), fpm(m, "m"), fpm(v, "v"), n, (float)lr,
                              (float)beta1, (float)beta2, (float)eps, step_count.data_ptr<int32_t>(), (float)max_norm,
                              fpm(grad_norm, "grad_norm"), aligned(ws), nb, stream_of(theta)),
        "adam_clip_step");
}

// {tile rows of the tape kernel, G, tail fused} of fabhip::buffer_train_step for this flow under the current options
std::vector<int64_t> train_step_plan(int64_t dim, int64_t n_layers, int64_t width) {
    std::vector<int64_t> out(3);
    chk(fabhip_train_step_plan((int32_t)dim, (int32_t)n_layers, (int32_t)width, out.data()), "train_step_plan");
    return out;
}

// One gradient step on one minibatch of the prioritised replay buffer (fab/train_with_prioritised_buffer.py:158-185) as ONE op:
// training pack, log q with the tape (the minibatch read in place from the buffer through `rows`), loss weights + buffer.adjust,
// parameter gradients, clipped Adam - nine launches, no host synchronisation, no autograd graph.  `pset`: the flow's registered
// parameter set (tensors_key_register: the order of fabhip_flow_params), whose tensors live inside `theta` (FlatAdam).
std::tuple<Tensor, Tensor, Tensor> buffer_train_step(int64_t pset, Tensor packed, int64_t dim, int64_t n_layers, int64_t width,
                                                     bool repack, const Tensor& x, const optional<Tensor>& rows,
                                                     const Tensor& log_q_old, bool log_q_old_rows, double alpha, double w_clip,
                                                     optional<Tensor> buf_log_w, optional<Tensor> buf_log_q_old, Tensor theta,
                                                     Tensor m, Tensor v, double lr, double beta1, double beta2, double eps,
                                                     Tensor step_count, double max_norm) {
    c10::DeviceGuard g(theta.device());
    fabhip_flow_params p;
    {
        std::lock_guard<std::mutex> lk(g_keysets_mu);
        TORCH_CHECK(pset >= 0 && pset < (int64_t)g_keysets.size() && !g_keysets[(size_t)pset].empty(),
                    "fabhip: unknown parameter-set handle ", pset);
        fill_params(p, g_keysets[(size_t)pset], dim, n_layers, width);
    }
    make_flow(packed, dim, n_layers, width);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [rows, dim]");
    const int64_t B = rows.has_value() ? rows->numel() : x.size(0);
    TORCH_CHECK(B >= 1, "fabhip: empty minibatch");
    if (rows.has_value()) need(*rows, at::kLong, "rows");
    TORCH_CHECK(buf_log_w.has_value() == buf_log_q_old.has_value(), "fabhip: buf_log_w and buf_log_q_old go together");
    TORCH_CHECK(!(buf_log_w.has_value() || log_q_old_rows) || rows.has_value(), "fabhip: in-place buffer access needs `rows`");
    const int64_t n_rows = x.size(0);
    if (log_q_old_rows) need_n(log_q_old, n_rows, theta, "log_q_old (the buffer's)");
    else need_n(log_q_old, B, theta, "log_q_old");
    const int64_t n = theta.numel();
    TORCH_CHECK(m.numel() == n && v.numel() == n, "fabhip: adam image sizes differ");
    need(step_count, at::kInt, "step_count");
    int64_t lay[15];
    chk(fabhip_flow_grad_layout((int32_t)dim, (int32_t)n_layers, (int32_t)width, lay), "flow_grad_layout");
    TORCH_CHECK(n == (p.an_s[0] ? lay[14] : lay[12]), "fabhip: theta has ", n, " floats, the flow's flat layout ", lay[12]);
    // (the parameters must be views of theta: the gradient image and the Adam step use its layout)
    TORCH_CHECK(p.w1[0] == theta.data_ptr<float>() + lay[1], "fabhip: the flow's parameters do not live inside theta (FlatAdam)");
    Tensor log_q = fempty({B}, theta), adj = fempty({B}, theta), coef = fempty({B}, theta), grads = fempty({n}, theta),
           stats = fempty({8}, theta);                      // (every entry is written by the step's kernels)
    const size_t nb = fabhip_train_step_workspace_bytes((int32_t)dim, (int32_t)n_layers, (int32_t)width, B, n);
    TORCH_CHECK(nb > 0, "fabhip: flow shape not supported");
    Tensor ws = scratch(nb, theta);
    fabhip_train_step_args a;
    a.struct_bytes = sizeof(a);
    a.params = &p; a.packed = packed.data_ptr<float>(); a.repack = repack ? 1 : 0; a.log_q_old_rows = log_q_old_rows ? 1 : 0;
    a.x = fp(x, "x"); a.rows = rows.has_value() ? rows->data_ptr<int64_t>() : nullptr; a.log_q_old = fp(log_q_old, "log_q_old");
    a.B = B; a.alpha = (float)alpha; a.w_adjust_max_clip = (float)w_clip;
    a.buf_log_w = buf_log_w.has_value() ? fpmn(*buf_log_w, n_rows, theta, "buffer log_w") : nullptr;
    a.buf_log_q_old = buf_log_q_old.has_value() ? fpmn(*buf_log_q_old, n_rows, theta, "buffer log_q_old") : nullptr;
    a.log_q = log_q.data_ptr<float>(); a.log_w_adjust = adj.data_ptr<float>(); a.coef = coef.data_ptr<float>();
    a.grads = grads.data_ptr<float>(); a.stats = stats.data_ptr<float>();
    a.theta = fpm(theta, "theta"); a.m = fpm(m, "m"); a.v = fpm(v, "v"); a.n_params = n;
    a.lr = (float)lr; a.beta1 = (float)beta1; a.beta2 = (float)beta2; a.eps = (float)eps; a.max_grad_norm = (float)max_norm;
    a.step_count = step_count.data_ptr<int32_t>();
    a.workspace = aligned(ws); a.workspace_bytes = nb;
    chk(fabhip_buffer_train_step(&a, stream_of(theta)), "buffer_train_step");
    return {log_q, adj, stats};
}

// ------------------------------------------------------------------------------------------------------------------
// RQ-spline coupling flow.  `Tensor[] params`: per layer {meta, w0, b0, wa, ba, wb, bb, wf, bf, pfw, uw, uh, ud}
// (pfw may be an empty tensor), then {base_scale, base_circ}.
// ------------------------------------------------------------------------------------------------------------------
fabhip_spline_flow make_spline(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t hidden, int64_t precision = 0) {
    fabhip_spline_flow f;
    TORCH_CHECK(precision >= 0 && precision <= 2, "fabhip: precision must be 0 (process default), 1 (fp32) or 2 (fast)");
    f.dim = (int32_t)dim; f.n_layers = (int32_t)n_layers; f.hidden = (int32_t)hidden; f.precision = (int32_t)precision;
    f.packed = fp(packed, "packed spline image");
    const int64_t n = fabhip_spline_packed_floats(f.dim, f.n_layers, f.hidden);
    TORCH_CHECK(n > 0, "fabhip: spline flow shape not supported (dim ", dim, ", hidden ", hidden, ")");
    TORCH_CHECK(packed.numel() == n, "fabhip: packed spline image has ", packed.numel(), " floats, expected ", n);
    return f;
}

void spline_pack(at::TensorList params, int64_t dim, int64_t n_layers, int64_t hidden, Tensor packed) {
    c10::DeviceGuard g(packed.device());
    TORCH_CHECK(n_layers >= 1 && n_layers <= FABHIP_MAX_LAYERS, "fabhip: n_layers out of range");
    TORCH_CHECK((int64_t)params.size() == 13 * n_layers + 2, "fabhip: expected ", 13 * n_layers + 2, " spline tensors");
    make_spline(packed, dim, n_layers, hidden);
    fabhip_spline_params p;
    p.dim = (int32_t)dim; p.n_layers = (int32_t)n_layers; p.hidden = (int32_t)hidden;
    for (int64_t l = 0; l < n_layers; ++l) {
        const Tensor* t = &params[13 * l];
        p.meta[l] = fp(t[0], "meta"); p.w0[l] = fp(t[1], "w0"); p.b0[l] = fp(t[2], "b0"); p.wa[l] = fp(t[3], "wa");
        p.ba[l] = fp(t[4], "ba"); p.wb[l] = fp(t[5], "wb"); p.bb[l] = fp(t[6], "bb"); p.wf[l] = fp(t[7], "wf");
        p.bf[l] = fp(t[8], "bf"); p.pfw[l] = t[9].numel() ? fp(t[9], "pfw") : nullptr;
        p.uw[l] = fp(t[10], "uw"); p.uh[l] = fp(t[11], "uh"); p.ud[l] = fp(t[12], "ud");
        TORCH_CHECK(t[0].numel() == 12 * 64, "fabhip: spline meta must be [12, 64]");
    }
    p.base_scale = fp(params[13 * n_layers], "base_scale");
    p.base_circ = fp(params[13 * n_layers + 1], "base_circ");
    chk(fabhip_spline_pack(&p, packed.data_ptr<float>(), stream_of(packed)), "spline_pack");
}

std::tuple<Tensor, Tensor> spline_logprob_grad(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t hidden,
                                               const Tensor& x, bool with_grad, int64_t precision) {
    c10::DeviceGuard g(x.device());
    const fabhip_spline_flow f = make_spline(packed, dim, n_layers, hidden, precision);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [B, dim]");
    const int64_t B = x.size(0);
    Tensor log_q = fempty({B}, x), grad = with_grad ? at::empty_like(x) : fempty({0}, x);
    const size_t nb = fabhip_spline_workspace_bytes(f.dim, f.n_layers, f.hidden, B, with_grad ? 1 : 0);
    Tensor ws = scratch(nb, x);
    chk(fabhip_spline_log_prob(&f, fp(x, "x"), log_q.data_ptr<float>(), with_grad ? grad.data_ptr<float>() : nullptr, B,
                               aligned(ws), nb, stream_of(x)),
        "spline_log_prob");
    return {log_q, grad};
}

std::vector<int64_t> spline_tape_layout(int64_t dim, int64_t n_layers, int64_t hidden, int64_t B) {
    std::vector<int64_t> out(16);
    chk(fabhip_spline_tape_layout((int32_t)dim, (int32_t)n_layers, (int32_t)hidden, B, out.data()), "spline_tape_layout");
    return out;
}

// log_q, d log_q / dx and the training tape (see fabhip_spline_tape_layout); the parameter gradients are GEMMs over
// tape slices done in fab_torch_amd/spline_flow.py
std::tuple<Tensor, Tensor, Tensor> spline_logprob_tape(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t hidden,
                                                       const Tensor& x) {
    c10::DeviceGuard g(x.device());
    const fabhip_spline_flow f = make_spline(packed, dim, n_layers, hidden);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [B, dim]");
    const int64_t B = x.size(0);
    int64_t lay[16];
    chk(fabhip_spline_tape_layout(f.dim, f.n_layers, f.hidden, B, lay), "spline_tape_layout");
    Tensor log_q = fempty({B}, x), grad = at::empty_like(x), tape = fempty({lay[0]}, x);
    const size_t nb = fabhip_spline_workspace_bytes(f.dim, f.n_layers, f.hidden, B, 1);
    Tensor ws = scratch(nb, x);
    chk(fabhip_spline_log_prob_tape(&f, fp(x, "x"), log_q.data_ptr<float>(), grad.data_ptr<float>(), B,
                                    tape.data_ptr<float>(), lay[0], aligned(ws), nb, stream_of(x)),
        "spline_log_prob_tape");
    return {log_q, grad, tape};
}

// the backward of flow.sample_and_log_prob (fabhip_spline_sample_vjp_tape): the two tapes for the tape GEMMs (coefficients gl and
// 1) and v at the base side
std::tuple<Tensor, Tensor, Tensor> spline_sample_vjp_tape(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t hidden,
                                                          const Tensor& u, const Tensor& eps, const optional<Tensor>& gx,
                                                          const optional<Tensor>& gl) {
    c10::DeviceGuard g(u.device());
    const fabhip_spline_flow f = make_spline(packed, dim, n_layers, hidden);
    TORCH_CHECK(u.dim() == 2 && u.size(1) == dim && eps.sizes() == u.sizes(), "fabhip: u, eps must be [B, dim]");
    TORCH_CHECK(!gx.has_value() || gx->sizes() == u.sizes(), "fabhip: gx must be [B, dim]");
    const int64_t B = u.size(0);
    TORCH_CHECK(!gl.has_value() || (gl->dim() == 1 && gl->size(0) == B), "fabhip: gl must be [B]");
    int64_t lay[16];
    chk(fabhip_spline_tape_layout(f.dim, f.n_layers, f.hidden, B, lay), "spline_tape_layout");
    Tensor tape1 = fempty({lay[0]}, u), tape2 = fempty({lay[0]}, u), v_x = at::empty_like(u), v_base = at::empty_like(u);
    const size_t nb = fabhip_spline_workspace_bytes(f.dim, f.n_layers, f.hidden, B, 1);
    Tensor ws = scratch(nb, u);
    chk(fabhip_spline_sample_vjp_tape(&f, fp(u, "u"), fp(eps, "eps"), fp_opt(gx, "gx"), fp_opt(gl, "gl"), v_x.data_ptr<float>(),
                                      v_base.data_ptr<float>(), B, tape1.data_ptr<float>(), tape2.data_ptr<float>(), lay[0],
                                      aligned(ws), nb, stream_of(u)),
        "spline_sample_vjp_tape");
    return {tape1, tape2, v_base};
}

std::tuple<Tensor, Tensor> spline_sample(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t hidden,
                                         const Tensor& u, const Tensor& eps) {
    c10::DeviceGuard g(u.device());
    const fabhip_spline_flow f = make_spline(packed, dim, n_layers, hidden);
    TORCH_CHECK(u.dim() == 2 && u.size(1) == dim && eps.sizes() == u.sizes(), "fabhip: u, eps must be [B, dim]");
    const int64_t B = u.size(0);
    Tensor x = at::empty_like(u), log_q = fempty({B}, u);
    const size_t nb = fabhip_spline_workspace_bytes(f.dim, f.n_layers, f.hidden, B, 0);
    Tensor ws = scratch(nb, u);
    chk(fabhip_spline_sample(&f, fp(u, "u"), fp(eps, "eps"), x.data_ptr<float>(), log_q.data_ptr<float>(), B, aligned(ws),
                             nb, stream_of(u)),
        "spline_sample");
    return {x, log_q};
}

// ------------------------------------------------------------------------------------------------------------------
// targets, points
// ------------------------------------------------------------------------------------------------------------------
std::tuple<Tensor, Tensor> target_logp_grad(int64_t kind, at::ArrayRef<double> prm, const optional<Tensor>& locs,
                                            const optional<Tensor>& scales, const Tensor& x, bool with_grad) {
    c10::DeviceGuard g(x.device());
    TORCH_CHECK(x.dim() == 2, "fabhip: x must be [B, dim]");
    const fabhip_target t = make_target(kind, prm, locs, scales, x.size(1), x);
    const int64_t B = x.size(0);
    Tensor lp = fempty({B}, x), grad = with_grad ? at::empty_like(x) : fempty({0}, x);
    chk(fabhip_target_log_prob(&t, fp(x, "x"), lp.data_ptr<float>(), with_grad ? grad.data_ptr<float>() : nullptr, B,
                               stream_of(x)),
        "target_log_prob");
    return {lp, grad};
}

std::tuple<Tensor, Tensor> manywell_logp_grad(const Tensor& x, double a, double b, double c, double log_norm) {
    const double prm[4] = {a, b, c, log_norm};
    return target_logp_grad(FABHIP_TARGET_MANYWELL, prm, c10::nullopt, c10::nullopt, x, true);
}

std::tuple<Tensor, Tensor> gmm_logp_grad(const Tensor& x, const Tensor& locs, const Tensor& scales) {
    const double prm[4] = {0, 0, 0, 0};
    return target_logp_grad(FABHIP_TARGET_GMM, prm, locs, scales, x, true);
}

std::tuple<Tensor, Tensor, Tensor, Tensor> create_point(const Tensor& packed, int64_t dim, int64_t n_layers,
                                                        int64_t width, int64_t kind, at::ArrayRef<double> prm,
                                                        const optional<Tensor>& locs, const optional<Tensor>& scales,
                                                        const Tensor& x, bool with_grad, int64_t precision) {
    c10::DeviceGuard g(x.device());
    const fabhip_flow f = make_flow(packed, dim, n_layers, width, precision);
    const fabhip_target t = make_target(kind, prm, locs, scales, dim, packed);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [B, dim]");
    const int64_t B = x.size(0);
    Tensor lq = fempty({B}, x), lp = fempty({B}, x);
    Tensor gq = with_grad ? at::empty_like(x) : fempty({0}, x), gp = with_grad ? at::empty_like(x) : fempty({0}, x);
    fabhip_point p{const_cast<float*>(fp(x, "x")), lq.data_ptr<float>(), lp.data_ptr<float>(),
                   with_grad ? gq.data_ptr<float>() : nullptr, with_grad ? gp.data_ptr<float>() : nullptr};
    chk(fabhip_create_point(&f, &t, &p, with_grad ? 1 : 0, B, stream_of(x)), "create_point");
    return {lq, lp, gq, gp};
}

// ------------------------------------------------------------------------------------------------------------------
// transitions (in place on the Point tensors, the step-size state and log_w)
// ------------------------------------------------------------------------------------------------------------------
void hmc_transition(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t kind,
                    at::ArrayRef<double> prm, const optional<Tensor>& locs, const optional<Tensor>& scales, Tensor x,
                    Tensor log_q, Tensor log_p, Tensor grad_log_q, Tensor grad_log_p, optional<Tensor> log_w,
                    double beta, double beta_next, double alpha, bool p_target, const Tensor& noise_p,
                    const Tensor& noise_e, Tensor epsilons_row, Tensor common_epsilon, const Tensor& mass, int64_t L,
                    double max_grad, double target_p_accept, bool tune, optional<Tensor> p_accept,
                    optional<Tensor> avg_distance, int64_t precision) {
    c10::DeviceGuard g(x.device());
    fabhip_hmc_args a;
    a.flow = make_flow(packed, dim, n_layers, width, precision);
    a.target = make_target(kind, prm, locs, scales, dim, packed);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [B, dim]");
    const int64_t B = x.size(0), n_outer = epsilons_row.numel();
    TORCH_CHECK(noise_p.numel() == n_outer * B * dim && noise_e.numel() == n_outer * B, "fabhip: HMC noise shapes");
    TORCH_CHECK(n_outer >= 1, "fabhip: epsilons row must hold one step size per outer loop");
    a.point = fabhip_point{fpm(x, "x"), fpmn(log_q, B, x, "log_q"), fpmn(log_p, B, x, "log_p"),
                           fpmn(grad_log_q, B * dim, x, "grad_log_q"), fpmn(grad_log_p, B * dim, x, "grad_log_p")};
    a.B = B; a.n_valid = nullptr;
    a.cur = coefs(beta, alpha, p_target); a.next = coefs(beta_next, alpha, p_target);
    a.log_w = fpmn_opt(log_w, B, x, "log_w");
    a.noise_p = fpn(noise_p, n_outer * B * dim, x, "noise_p"); a.noise_e = fpn(noise_e, n_outer * B, x, "noise_e");
    a.epsilons = fpmn(epsilons_row, n_outer, x, "epsilons");
    a.common_epsilon = fpmn(common_epsilon, 1, x, "common_epsilon", true);
    a.mass = fpn(mass, dim, x, "mass");
    a.n_outer = (int32_t)n_outer; a.L = (int32_t)L; a.max_grad = (float)max_grad;
    a.target_p_accept = (float)target_p_accept; a.tune = tune ? 1 : 0;
    a.p_accept = fpmn_opt(p_accept, n_outer, x, "p_accept", true);
    a.avg_distance = fpmn_opt(avg_distance, 1, x, "avg_distance", true);
    const size_t nb = fabhip_hmc_workspace_bytes(B, (int32_t)dim, (int32_t)n_outer);
    Tensor ws = scratch(nb, x);
    a.workspace = aligned(ws); a.workspace_bytes = nb;
    a.partials = nullptr;
    chk(fabhip_hmc_transition(&a, stream_of(x)), "hmc_transition");
}

void metropolis_transition(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t kind,
                           at::ArrayRef<double> prm, const optional<Tensor>& locs, const optional<Tensor>& scales,
                           Tensor x, Tensor log_q, Tensor log_p, optional<Tensor> log_w, double beta, double beta_next,
                           double alpha, bool p_target, const Tensor& noise_x, const Tensor& noise_u,
                           Tensor noise_scalings_row, double target_p_accept, bool tune) {
    c10::DeviceGuard g(x.device());
    fabhip_metropolis_args a;
    a.flow = make_flow(packed, dim, n_layers, width);
    a.target = make_target(kind, prm, locs, scales, dim, packed);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [B, dim]");
    const int64_t B = x.size(0), n_updates = noise_scalings_row.numel();
    TORCH_CHECK(noise_x.numel() == n_updates * B * dim && noise_u.numel() == n_updates * B,
                "fabhip: Metropolis noise shapes");
    TORCH_CHECK(n_updates >= 1, "fabhip: noise_scalings row must hold one scale per update");
    a.point = fabhip_point{fpm(x, "x"), fpmn(log_q, B, x, "log_q"), fpmn(log_p, B, x, "log_p"), nullptr, nullptr};
    a.B = B; a.n_valid = nullptr;
    a.cur = coefs(beta, alpha, p_target); a.next = coefs(beta_next, alpha, p_target);
    a.log_w = fpmn_opt(log_w, B, x, "log_w");
    a.noise_x = fpn(noise_x, n_updates * B * dim, x, "noise_x"); a.noise_u = fpn(noise_u, n_updates * B, x, "noise_u");
    a.noise_scalings = fpmn(noise_scalings_row, n_updates, x, "noise_scalings");
    a.n_updates = (int32_t)n_updates; a.target_p_accept = (float)target_p_accept; a.tune = tune ? 1 : 0;
    const size_t nb = fabhip_metropolis_workspace_bytes(B, (int32_t)dim, (int32_t)n_updates);
    Tensor ws = scratch(nb, x);
    a.workspace = aligned(ws); a.workspace_bytes = nb;
    chk(fabhip_metropolis_transition(&a, stream_of(x)), "metropolis_transition");
}

// ------------------------------------------------------------------------------------------------------------------
// generic plug-in path (any Distribution / LogProbFunc: densities + gradients evaluated by the caller)
// ------------------------------------------------------------------------------------------------------------------
Tensor generic_workspace(const Tensor& like, int64_t B, int64_t dim) {
    return at::empty({(int64_t)(fabhip_generic_workspace_bytes(B, (int32_t)dim) / 4 + 64)}, like.options().dtype(at::kFloat));
}
size_t ws_bytes(const Tensor& ws) { return (size_t)ws.numel() * 4; }

void hmc_generic_begin(const Tensor& start_x, const Tensor& start_gq, const Tensor& start_gp, const Tensor& cur_lq,
                       const Tensor& cur_lp, double beta, double alpha, bool p_target, const Tensor& noise_p,
                       const Tensor& mass, double max_grad, Tensor ws) {
    c10::DeviceGuard g(start_x.device());
    TORCH_CHECK(start_x.dim() == 2, "fabhip: x must be [B, dim]");
    const int64_t B = start_x.size(0), D = start_x.size(1);
    const Tensor& r = start_x;
    fabhip_point st{const_cast<float*>(fp(start_x, "x")), nullptr, nullptr,
                    const_cast<float*>(fpn(start_gq, B * D, r, "grad_log_q")),
                    const_cast<float*>(fpn(start_gp, B * D, r, "grad_log_p"))};
    fabhip_point cu{nullptr, const_cast<float*>(fpn(cur_lq, B, r, "log_q")), const_cast<float*>(fpn(cur_lp, B, r, "log_p")),
                    nullptr, nullptr};
    need_n(ws, 0, r, "workspace", true);
    chk(fabhip_hmc_generic_begin(&st, &cu, B, (int32_t)D, coefs(beta, alpha, p_target), fpn(noise_p, B * D, r, "noise_p"),
                                 fpn(mass, D, r, "mass"), (float)max_grad, fpm(ws, "workspace"), ws_bytes(ws), stream_of(start_x)),
        "hmc_generic_begin");
}

Tensor hmc_generic_leap_pre(int64_t B, int64_t dim, const Tensor& eps, const Tensor& ceps, const Tensor& mass,
                            Tensor ws) {
    c10::DeviceGuard g(ws.device());
    Tensor x = fempty({B, dim}, ws);
    need_n(eps, 1, ws, "epsilon", true); need_n(ceps, 1, ws, "common_epsilon", true); need_n(mass, dim, ws, "mass");
    chk(fabhip_hmc_generic_leap_pre(B, (int32_t)dim, fp(eps, "epsilon"), fp(ceps, "common_epsilon"), fp(mass, "mass"),
                                    x.data_ptr<float>(), fpm(ws, "workspace"), ws_bytes(ws), stream_of(ws)),
        "hmc_generic_leap_pre");
    return x;
}

void hmc_generic_leap_post(const Tensor& gq, const Tensor& gp, double beta, double alpha, bool p_target, double max_grad,
                           const Tensor& eps, const Tensor& ceps, Tensor ws) {
    c10::DeviceGuard g(ws.device());
    TORCH_CHECK(gq.dim() == 2, "fabhip: grad_log_q must be [B, dim]");
    const int64_t B = gq.size(0), D = gq.size(1);
    need_n(gq, B * D, ws, "grad_log_q"); need_n(gp, B * D, ws, "grad_log_p");
    need_n(eps, 1, ws, "epsilon", true); need_n(ceps, 1, ws, "common_epsilon", true);
    chk(fabhip_hmc_generic_leap_post(B, (int32_t)D, fp(gq, "grad_log_q"), fp(gp, "grad_log_p"),
                                     coefs(beta, alpha, p_target), (float)max_grad, fp(eps, "epsilon"),
                                     fp(ceps, "common_epsilon"), fpm(ws, "workspace"), ws_bytes(ws), stream_of(ws)),
        "hmc_generic_leap_post");
}

void hmc_generic_accept(const Tensor& prop_lq, const Tensor& prop_lp, const Tensor& prop_gq, const Tensor& prop_gp,
                        Tensor x, Tensor log_q, Tensor log_p, Tensor grad_log_q, Tensor grad_log_p,
                        optional<Tensor> log_w, double beta, double beta_next, double alpha, bool p_target,
                        const Tensor& noise_e, const Tensor& mass, Tensor eps, Tensor ceps, double target_p_accept,
                        bool tune, optional<Tensor> p_accept, optional<Tensor> avg_distance, Tensor ws) {
    c10::DeviceGuard g(x.device());
    TORCH_CHECK(x.dim() == 2, "fabhip: x must be [B, dim]");
    const int64_t B = x.size(0), D = x.size(1);
    fabhip_point pr{nullptr, const_cast<float*>(fpn(prop_lq, B, x, "log_q")), const_cast<float*>(fpn(prop_lp, B, x, "log_p")),
                    const_cast<float*>(fpn(prop_gq, B * D, x, "grad_log_q")),
                    const_cast<float*>(fpn(prop_gp, B * D, x, "grad_log_p"))};
    fabhip_point cu{fpm(x, "x"), fpmn(log_q, B, x, "log_q"), fpmn(log_p, B, x, "log_p"),
                    fpmn(grad_log_q, B * D, x, "grad_log_q"), fpmn(grad_log_p, B * D, x, "grad_log_p")};
    need_n(ws, 0, x, "workspace", true);
    chk(fabhip_hmc_generic_accept(&pr, &cu, B, (int32_t)D, coefs(beta, alpha, p_target), coefs(beta_next, alpha, p_target),
                                  fpmn_opt(log_w, B, x, "log_w"), fpn(noise_e, B, x, "noise_e"), fpn(mass, D, x, "mass"),
                                  fpmn(eps, 1, x, "epsilon", true), fpmn(ceps, 1, x, "common_epsilon", true),
                                  (float)target_p_accept, tune ? 1 : 0, fpmn_opt(p_accept, 1, x, "p_accept", true),
                                  fpmn_opt(avg_distance, 1, x, "avg_distance", true),
                                  fpm(ws, "workspace"), ws_bytes(ws), stream_of(x)),
        "hmc_generic_accept");
}

// One HMC transition (hmc.py:129-160, all n_outer x L leapfrogs) for the SPLINE flow + a native target, enqueued from
// C++: per leapfrog the generic element-wise kernels, the one-launch spline density + gradient kernel and the target
// kernel - what transition_operators.py::_transition_generic does step by step from Python, without the ~40 op calls
// per transition in between (they cost as much as the kernels at batch sizes <= 1024).
void spline_hmc_transition(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t hidden, int64_t kind,
                           at::ArrayRef<double> prm, const optional<Tensor>& locs, const optional<Tensor>& scales, Tensor x,
                           Tensor log_q, Tensor log_p, Tensor grad_log_q, Tensor grad_log_p, optional<Tensor> log_w,
                           double beta, double beta_next, double alpha, bool p_target, const Tensor& noise_p,
                           const Tensor& noise_e, Tensor eps_row, Tensor ceps, const Tensor& mass, int64_t n_outer,
                           int64_t n_leap, double max_grad, double target_p_accept, bool tune, optional<Tensor> p_accept,
                           optional<Tensor> avg_distance, int64_t precision) {
    c10::DeviceGuard g(x.device());
    const fabhip_spline_flow f = make_spline(packed, dim, n_layers, hidden, precision);
    const fabhip_target tg = make_target(kind, prm, locs, scales, dim, packed);
    TORCH_CHECK(x.dim() == 2, "fabhip: x must be [B, dim]");
    const int64_t B = x.size(0), D = x.size(1);
    TORCH_CHECK(D == dim && n_outer >= 1 && n_leap >= 1, "fabhip: spline_hmc_transition shapes");
    need_n(log_q, B, x, "log_q"); need_n(log_p, B, x, "log_p");
    need_n(grad_log_q, B * D, x, "grad_log_q"); need_n(grad_log_p, B * D, x, "grad_log_p");
    if (log_w.has_value()) need_n(*log_w, B, x, "log_w");
    need_n(noise_p, n_outer * B * D, x, "noise_p"); need_n(noise_e, n_outer * B, x, "noise_e");
    need_n(eps_row, n_outer, x, "epsilons"); need_n(ceps, 1, x, "common_epsilon", true); need_n(mass, D, x, "mass");
    if (p_accept.has_value()) need_n(*p_accept, n_outer, x, "p_accept", true);
    if (avg_distance.has_value()) need_n(*avg_distance, 1, x, "avg_distance", true);
    if (B == 0) return;
    fabhip_spline_hmc_args a;
    a.flow = f; a.target = tg;
    a.point = fabhip_point{fpm(x, "x"), fpm(log_q, "log_q"), fpm(log_p, "log_p"), fpm(grad_log_q, "grad_log_q"),
                           fpm(grad_log_p, "grad_log_p")};
    a.B = B; a.n_valid = nullptr;
    a.cur = coefs(beta, alpha, p_target); a.next = coefs(beta_next, alpha, p_target);
    a.log_w = fpm_opt(log_w, "log_w");
    a.noise_p = fp(noise_p, "noise_p"); a.noise_e = fp(noise_e, "noise_e");
    a.epsilons = fpm(eps_row, "epsilons"); a.common_epsilon = fpm(ceps, "common_epsilon"); a.mass = fp(mass, "mass");
    a.n_outer = (int32_t)n_outer; a.L = (int32_t)n_leap; a.max_grad = (float)max_grad;
    a.target_p_accept = (float)target_p_accept; a.tune = tune ? 1 : 0;
    a.p_accept = fpm_opt(p_accept, "p_accept"); a.avg_distance = fpm_opt(avg_distance, "avg_distance");
    const size_t nb = fabhip_spline_hmc_workspace_bytes(f.dim, f.n_layers, f.hidden, B);
    Tensor ws = scratch(nb, x);
    a.workspace = aligned(ws); a.workspace_bytes = nb;
    chk(fabhip_spline_hmc_transition(&a, stream_of(x)), "spline_hmc_transition");
}

// What the whole-call AIS ops (ais_run, ais_run_ext, spline_ais_run) and their argument structs have in common.
// The four logging slots (hmc.py:173-183, store_info): at least n_inner / 1 floats each.
template <class Args>
void fill_logging_slots(Args& a, int64_t n_inner, const Tensor& ref, const optional<Tensor>& p_accept_first,
                        const optional<Tensor>& p_accept_last, const optional<Tensor>& avg_distance_first,
                        const optional<Tensor>& avg_distance_last) {
    a.p_accept_first = fpmn_opt(p_accept_first, n_inner, ref, "p_accept_first", true);
    a.p_accept_last = fpmn_opt(p_accept_last, n_inner, ref, "p_accept_last", true);
    a.avg_distance_first = fpmn_opt(avg_distance_first, 1, ref, "avg_distance_first", true);
    a.avg_distance_last = fpmn_opt(avg_distance_last, 1, ref, "avg_distance_last", true);
}
// The outputs besides the Point and log_w: stats[16] | n_valid[2] as views of ONE 18-word buffer (one device->host copy,
// _ops.read_counts_and_stats; every word is written by the call: the counts and statistics by the phase tails, stats[6..15] = 0)
// and, with want_base, the chains' starting points and their log p - log q.
struct AisOutputs { Tensor stats, n_valid, base_x, base_lw; };
template <class Args>
AisOutputs alloc_ais_outputs(Args& a, int64_t B, int64_t dim, const Tensor& like, bool want_base) {
    Tensor counts_stats = at::empty({18}, like.options());
    AisOutputs o{counts_stats.narrow(0, 0, 16), counts_stats.narrow(0, 16, 2).view(at::kInt),
                 want_base ? fempty({B, dim}, like) : fempty({0}, like), want_base ? fempty({B}, like) : fempty({0}, like)};
    a.n_valid = o.n_valid.data_ptr<int32_t>(); a.stats = o.stats.data_ptr<float>();
    a.base_x = want_base ? o.base_x.data_ptr<float>() : nullptr;
    a.base_log_w = want_base ? o.base_lw.data_ptr<float>() : nullptr;
    return o;
}

// The spline family's ais_run (fabhip_spline_ais_run): same outputs as ais_run.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> spline_ais_run(
    const Tensor& packed, int64_t dim, int64_t n_layers, int64_t hidden, int64_t kind, at::ArrayRef<double> prm,
    const optional<Tensor>& locs, const optional<Tensor>& scales, at::ArrayRef<double> betas, double alpha, bool p_target,
    const Tensor& u0, const Tensor& eps0, const Tensor& noise_p, const Tensor& noise_e, Tensor epsilons, Tensor common_epsilon,
    const Tensor& mass, int64_t n_outer, int64_t L, double max_grad, double target_p_accept, bool tune,
    optional<Tensor> p_accept_first, optional<Tensor> p_accept_last, optional<Tensor> avg_distance_first,
    optional<Tensor> avg_distance_last, bool want_base, int64_t precision) {
    c10::DeviceGuard g(eps0.device());
    fabhip_spline_ais_args a;
    a.flow = make_spline(packed, dim, n_layers, hidden, precision);
    a.target = make_target(kind, prm, locs, scales, dim, packed);
    TORCH_CHECK(eps0.dim() == 2 && eps0.size(1) == dim, "fabhip: eps0 must be [B, dim]");
    const int64_t B = eps0.size(0), M = (int64_t)betas.size() - 2;
    TORCH_CHECK(M >= 1 && n_outer >= 1 && L >= 1, "fabhip: spline_ais_run needs M, n_outer, L >= 1");
    a.B = B; a.M = (int32_t)M;
    std::vector<double> bt(betas.begin(), betas.end());
    a.betas = bt.data(); a.alpha = alpha; a.p_target = p_target ? 1 : 0;
    a.u0 = fpn(u0, B * dim, eps0, "u0"); a.eps0 = fp(eps0, "eps0");
    a.noise_p = fpn(noise_p, M * n_outer * B * dim, eps0, "noise_p"); a.noise_e = fpn(noise_e, M * n_outer * B, eps0, "noise_e");
    a.epsilons = fpmn(epsilons, M * n_outer, eps0, "epsilons");
    a.common_epsilon = fpmn(common_epsilon, 1, eps0, "common_epsilon", true);
    a.mass = fpn(mass, dim, eps0, "mass");
    a.n_outer = (int32_t)n_outer; a.L = (int32_t)L; a.max_grad = (float)max_grad;
    a.target_p_accept = (float)target_p_accept; a.tune = tune ? 1 : 0;
    Tensor x = fempty({B, dim}, eps0), lq = fempty({B}, eps0), lp = fempty({B}, eps0), log_w = fempty({B}, eps0);
    Tensor gq = fempty({B, dim}, eps0), gp = fempty({B, dim}, eps0);
    a.point = fabhip_point{x.data_ptr<float>(), lq.data_ptr<float>(), lp.data_ptr<float>(), gq.data_ptr<float>(),
                           gp.data_ptr<float>()};
    a.log_w = log_w.data_ptr<float>();
    const AisOutputs o = alloc_ais_outputs(a, B, dim, eps0, want_base);
    fill_logging_slots(a, n_outer, eps0, p_accept_first, p_accept_last, avg_distance_first, avg_distance_last);
    const size_t nb = fabhip_spline_ais_workspace_bytes(a.flow.dim, a.flow.n_layers, a.flow.hidden, B);
    Tensor ws = scratch(nb, eps0);
    a.workspace = aligned(ws); a.workspace_bytes = nb;
    chk(fabhip_spline_ais_run(&a, stream_of(eps0)), "spline_ais_run");
    return {x, lq, lp, gq, gp, log_w, o.n_valid, o.stats, o.base_x, o.base_lw};
}

Tensor anneal_log_prob(const Tensor& log_q, const Tensor& log_p, double beta, double alpha, bool p_target) {
    c10::DeviceGuard g(log_q.device());
    Tensor out = at::empty_like(log_q);
    need_n(log_p, log_q.numel(), log_q, "log_p");
    chk(fabhip_anneal_log_prob(fp(log_q, "log_q"), fp(log_p, "log_p"), log_q.numel(), coefs(beta, alpha, p_target),
                               out.data_ptr<float>(), stream_of(log_q)),
        "anneal_log_prob");
    return out;
}

void log_w_update(const Tensor& log_q, const Tensor& log_p, double beta, double beta_next, double alpha, bool p_target,
                  Tensor log_w) {
    c10::DeviceGuard g(log_q.device());
    need_n(log_p, log_q.numel(), log_q, "log_p"); need_n(log_w, log_q.numel(), log_q, "log_w");
    chk(fabhip_log_w_update(fp(log_q, "log_q"), fp(log_p, "log_p"), log_q.numel(), coefs(beta, alpha, p_target),
                            coefs(beta_next, alpha, p_target), fpm(log_w, "log_w"), stream_of(log_q)),
        "log_w_update");
}

// The first weight of a chain whose initialisation ran at beta = 0 (fabhip_log_w_first; adaptive schedules).
void log_w_first(const Tensor& log_q, const Tensor& log_p, double beta_next, double alpha, bool p_target, Tensor log_w) {
    c10::DeviceGuard g(log_q.device());
    need_n(log_p, log_q.numel(), log_q, "log_p"); need_n(log_w, log_q.numel(), log_q, "log_w");
    chk(fabhip_log_w_first(fp(log_q, "log_q"), fp(log_p, "log_p"), log_q.numel(), coefs(beta_next, alpha, p_target),
                           fpm(log_w, "log_w"), stream_of(log_q)),
        "log_w_first");
}

Tensor metropolis_generic_propose(const Tensor& x, const Tensor& noise_x, const Tensor& scale) {
    c10::DeviceGuard g(x.device());
    Tensor xn = at::empty_like(x);
    TORCH_CHECK(x.dim() == 2, "fabhip: x must be [B, dim]");
    need_n(noise_x, x.numel(), x, "noise_x"); need_n(scale, 1, x, "noise_scaling", true);
    chk(fabhip_metropolis_generic_propose(fp(x, "x"), fp(noise_x, "noise_x"), fp(scale, "noise_scaling"), x.size(0),
                                          (int32_t)x.size(1), xn.data_ptr<float>(), stream_of(x)),
        "metropolis_generic_propose");
    return xn;
}

void metropolis_generic_accept(const Tensor& x_new, const Tensor& new_lq, const Tensor& new_lp, Tensor x, Tensor log_q,
                               Tensor log_p, const Tensor& prev_log_prob, const Tensor& noise_u, double beta, double alpha,
                               bool p_target, Tensor scale, double target_p_accept, bool tune) {
    c10::DeviceGuard g(x.device());
    TORCH_CHECK(x.dim() == 2, "fabhip: x must be [B, dim]");
    const int64_t B = x.size(0), D = x.size(1);
    fabhip_point cu{fpm(x, "x"), fpmn(log_q, B, x, "log_q"), fpmn(log_p, B, x, "log_p"), nullptr, nullptr};
    need_n(x_new, B * D, x, "x_new"); need_n(new_lq, B, x, "new log_q"); need_n(new_lp, B, x, "new log_p");
    need_n(prev_log_prob, B, x, "prev_log_prob"); need_n(noise_u, B, x, "noise_u"); need_n(scale, 1, x, "noise_scaling", true);
    Tensor ws = generic_workspace(x, B, D);
    chk(fabhip_metropolis_generic_accept(fp(x_new, "x_new"), fp(new_lq, "log_q"), fp(new_lp, "log_p"), &cu,
                                         fp(prev_log_prob, "prev_log_prob"), fp(noise_u, "noise_u"), B, (int32_t)D,
                                         coefs(beta, alpha, p_target), fpm(scale, "noise_scaling"),
                                         (float)target_p_accept, tune ? 1 : 0, fpm(ws, "workspace"), ws_bytes(ws),
                                         stream_of(x)),
        "metropolis_generic_accept");
}

// ------------------------------------------------------------------------------------------------------------------
// the whole AIS call (ais.py:53-105): returns
//   (x, log_q, log_p, grad_log_q, grad_log_p, log_w, n_valid int32[2], stats float[16], base_x, base_log_w)
// grad_* are empty for Metropolis, base_* are empty unless want_base.
// ------------------------------------------------------------------------------------------------------------------
// fabhip_ais_args and what it points to for the length of the C call.  `fill_ais_args` writes the part every AIS op shares;
// the op adds the noise and the state tensors (the ones it allocates, or the caller's).
struct AisCall {
    fabhip_ais_args a;
    std::vector<double> betas;      // a.betas
    Tensor ws;                      // a.workspace
    int64_t B = 0, M = 0;
    bool hmc = false;
    AisCall() = default;
    AisCall(const AisCall&) = delete;               // (a.betas points into this object's vector)
    AisCall& operator=(const AisCall&) = delete;
};

// flow, target, B / M / betas, alpha / p_target / transition, the operator's step state and settings, the logging slots and the
// workspace (`ext`: with the share of each mode that is on).  `ref`: the tensor whose device and stream the call is enqueued on.
void fill_ais_args(AisCall& c, const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t kind,
                   at::ArrayRef<double> prm, const optional<Tensor>& locs, const optional<Tensor>& scales,
                   at::ArrayRef<double> betas, double alpha, bool p_target, int64_t transition, int64_t B, const Tensor& ref,
                   const Tensor& step_state, const optional<Tensor>& common_epsilon, const optional<Tensor>& mass,
                   int64_t n_inner, int64_t L, double max_grad, double target_p_accept, bool tune,
                   const optional<Tensor>& p_accept_first, const optional<Tensor>& p_accept_last,
                   const optional<Tensor>& avg_distance_first, const optional<Tensor>& avg_distance_last, int64_t precision,
                   const fabhip_ais_ext* ext) {
    fabhip_ais_args& a = c.a;
    a.flow = make_flow(packed, dim, n_layers, width, precision);
    a.target = make_target(kind, prm, locs, scales, dim, packed);
    const int64_t M = (int64_t)betas.size() - 2;
    const bool hmc = transition == FABHIP_TRANSITION_HMC;
    TORCH_CHECK(M >= 1, "fabhip: betas must hold M + 2 values");
    TORCH_CHECK(n_inner >= 1, "fabhip: n_inner (HMC outer loops / Metropolis updates per transition) must be >= 1");
    TORCH_CHECK(hmc || transition == FABHIP_TRANSITION_METROPOLIS, "fabhip: unknown transition kind ", transition);
    TORCH_CHECK(!hmc || (common_epsilon.has_value() && mass.has_value()),
                "fabhip: an HMC AIS run needs common_epsilon and the mass vector");
    c.B = B; c.M = M; c.hmc = hmc;
    c.betas.assign(betas.begin(), betas.end());
    a.B = B; a.M = (int32_t)M; a.betas = c.betas.data();
    a.alpha = alpha; a.p_target = p_target ? 1 : 0; a.transition = (int32_t)transition;
    a.eps0 = a.noise_a = a.noise_b = nullptr;
    a.step_state = fpmn(step_state, M * n_inner, ref, "step_state");
    a.common_epsilon = fpmn_opt(common_epsilon, 1, ref, "common_epsilon", true);
    a.mass = mass.has_value() ? fpn(*mass, dim, ref, "mass") : nullptr;
    a.n_inner = (int32_t)n_inner; a.L = (int32_t)L; a.max_grad = (float)max_grad;
    a.target_p_accept = (float)target_p_accept; a.tune = tune ? 1 : 0;
    fill_logging_slots(a, n_inner, ref, p_accept_first, p_accept_last, avg_distance_first, avg_distance_last);
    const size_t nb = fabhip_ais_ext_workspace_bytes(B, (int32_t)dim, (int32_t)n_inner, ext);
    c.ws = scratch(nb, ref);
    a.workspace = aligned(c.ws); a.workspace_bytes = nb;
}

// Defensive-mixture base distribution of the AIS ops (fabhip_defensive_args): the module's three parameter tensors as they are
// (the kernels read them; no copy, no host read) and the branch uniforms `sel` [B] (absent: drawn from the default generator).
struct MixOp {
    bool enabled = true;
    Tensor loc, log_scale, logit;
    optional<Tensor> sel;
};
// Flow-proposal moves of the AIS ops (fabhip_flow_moves_args): n_moves moves in front of every transition.  noise_g [M, k, B, dim]
// / noise_h [M, k, B] absent: drawn from the default generator AFTER the transition noise, g before h (and before noise_r).
struct MovesOp {
    int64_t n_moves = 0;
    optional<Tensor> noise_g, noise_h;
    Tensor g, h, p_accept;                              // the draws the call used; out: acceptance fractions [M, k]
};
// SMC mode of the AIS ops (fabhip_smc_args).  noise_r [M] float64 (absent: drawn from the default generator AFTER the transition
// noise); the per-transition records are allocated here.
struct SmcOp {
    double tau = 0.0;
    optional<Tensor> noise_r;
    bool want_trace = false;
    int64_t method = 0;                                 // FABHIP_SMC_SYSTEMATIC / FABHIP_SMC_STRATIFIED
    Tensor resampled, ess, ancestors, log_w_pre, u;     // out
};
// The optional modes of one AIS op call (fabhip_ais_ext), each absent = not named.  The next mode is one more member here and one
// more parameter group of ais_run_ext.
struct AisExtOp {
    optional<SmcOp> smc;
    optional<MixOp> mix;
    optional<MovesOp> moves;
};

fabhip_defensive_args make_mix(const MixOp& m, int64_t dim, const Tensor& ref) {
    fabhip_defensive_args d = {};
    d.enabled = m.enabled ? 1 : 0;
    d.loc = fpn(m.loc, dim, ref, "loc"); d.log_scale = fpn(m.log_scale, dim, ref, "log_scale");
    d.logit = fpn(m.logit, 1, ref, "mixture_logit");
    return d;
}

static Tensor smc_uniforms(const optional<Tensor>& noise_r, int64_t M, const Tensor& like) {
    if (!noise_r.has_value()) return at::rand({M}, like.options().dtype(at::kDouble));
    need(*noise_r, at::kDouble, "noise_r");
    TORCH_CHECK(noise_r->dim() == 1 && noise_r->numel() == M && noise_r->is_contiguous() && noise_r->device() == like.device(),
                "fabhip: noise_r must be a contiguous float64 tensor [M] on the call's device");
    return *noise_r;
}

// `ext` == nullptr: the plain op (ais_run) - the entry points of ais_run_ext with a NULL fabhip_ais_ext.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> ais_run_impl(
    AisExtOp* ext, const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t kind, at::ArrayRef<double> prm,
    const optional<Tensor>& locs, const optional<Tensor>& scales, at::ArrayRef<double> betas, double alpha,
    bool p_target, int64_t transition, const Tensor& eps0, const optional<Tensor>& noise_a_in,
    const optional<Tensor>& noise_b_in, Tensor step_state, optional<Tensor> common_epsilon, const optional<Tensor>& mass,
    int64_t n_inner, int64_t L, double max_grad, double target_p_accept, bool tune, optional<Tensor> p_accept_first,
    optional<Tensor> p_accept_last, optional<Tensor> avg_distance_first, optional<Tensor> avg_distance_last, bool want_base,
    int64_t precision) {
    c10::DeviceGuard g(eps0.device());
    SmcOp* smc = ext != nullptr && ext->smc.has_value() ? &*ext->smc : nullptr;
    const MixOp* mix = ext != nullptr && ext->mix.has_value() ? &*ext->mix : nullptr;
    MovesOp* mv = ext != nullptr && ext->moves.has_value() ? &*ext->moves : nullptr;
    // noise_a / noise_b absent: drawn HERE, from the default generator in the order the Python side draws them (normal
    // [M, n_inner, B, dim], then exponential(1) / uniform [M, n_inner, B]) - but AFTER the chain initialisation is enqueued, so the
    // device works while the host launches the draws (FABHIP_AIS_CONTINUE)
    TORCH_CHECK(noise_a_in.has_value() == noise_b_in.has_value(), "fabhip: pass both noise tensors or neither");
    const bool draw_inside = !noise_a_in.has_value();
    TORCH_CHECK(eps0.dim() == 2 && eps0.size(1) == dim, "fabhip: eps0 must be [B, dim]");
    // the C structs of the modes: their switches now (the workspace is sized by them), their tensors where the generator's order
    // of draws puts them
    fabhip_smc_args sa = {};                                   // (records: NULL until smc_outputs)
    fabhip_defensive_args ma = {};
    fabhip_flow_moves_args fm = {};
    if (smc != nullptr) { sa.enabled = 1; sa.tau = smc->tau; sa.method = (int32_t)smc->method; }
    if (mix != nullptr) ma.enabled = mix->enabled ? 1 : 0;
    if (mv != nullptr) fm.n_moves = (int32_t)mv->n_moves;
    const fabhip_ais_ext whole = {smc != nullptr ? &sa : nullptr, mix != nullptr ? &ma : nullptr, mv != nullptr ? &fm : nullptr};
    const fabhip_ais_ext* xp = ext != nullptr ? &whole : nullptr;
    AisCall c;
    fill_ais_args(c, packed, dim, n_layers, width, kind, prm, locs, scales, betas, alpha, p_target, transition, eps0.size(0), eps0,
                  step_state, common_epsilon, mass, n_inner, L, max_grad, target_p_accept, tune, p_accept_first, p_accept_last,
                  avg_distance_first, avg_distance_last, precision, xp);
    fabhip_ais_args& a = c.a;
    const int64_t B = c.B, M = c.M;
    const bool hmc = c.hmc;
    a.eps0 = fp(eps0, "eps0");
    Tensor noise_a, noise_b;
    if (!draw_inside) {
        noise_a = *noise_a_in; noise_b = *noise_b_in;
        a.noise_a = fpn(noise_a, M * n_inner * B * dim, eps0, "noise_a"); a.noise_b = fpn(noise_b, M * n_inner * B, eps0, "noise_b");
    }
    // the outputs are views of ONE allocation (each padded to 256 bytes): one trip through the caching allocator instead of six
    // on the host path the GPU waits for
    auto pad64 = [](int64_t n) { return (n + 63) / 64 * 64; };
    Tensor pool = fempty({(hmc ? 3 : 1) * pad64(B * dim) + 3 * pad64(B)}, eps0);
    int64_t pool_off = 0;
    auto take = [&](int64_t rows, int64_t cols) {
        Tensor t = cols > 0 ? pool.narrow(0, pool_off, rows * cols).view({rows, cols}) : pool.narrow(0, pool_off, rows);
        pool_off += pad64(rows * (cols > 0 ? cols : 1));
        return t;
    };
    Tensor x = take(B, dim), lq = take(B, 0), lp = take(B, 0), log_w = take(B, 0);
    Tensor gq = hmc ? take(B, dim) : fempty({0}, eps0), gp = hmc ? take(B, dim) : fempty({0}, eps0);
    a.point = fabhip_point{x.data_ptr<float>(), lq.data_ptr<float>(), lp.data_ptr<float>(),
                           hmc ? gq.data_ptr<float>() : nullptr, hmc ? gp.data_ptr<float>() : nullptr};
    a.log_w = log_w.data_ptr<float>();
    const AisOutputs o = alloc_ais_outputs(a, B, dim, eps0, want_base);
    auto smc_outputs = [&]() {                                 // (after the transition noise: the generator's order of draws)
        if (smc == nullptr) return;
        smc->u = smc_uniforms(smc->noise_r, M, eps0);
        smc->resampled = at::empty({M}, eps0.options().dtype(at::kInt));
        smc->ess = fempty({M}, eps0);
        sa.u = smc->u.data_ptr<double>(); sa.resampled = smc->resampled.data_ptr<int32_t>(); sa.ess = smc->ess.data_ptr<float>();
        if (smc->want_trace) {
            smc->ancestors = at::empty({M, B}, eps0.options().dtype(at::kInt));
            smc->log_w_pre = fempty({M, B}, eps0);
            sa.ancestors = smc->ancestors.data_ptr<int32_t>(); sa.log_w_pre = smc->log_w_pre.data_ptr<float>();
        }
    };
    auto moves_noise = [&]() {                                 // (behind the transition noise, in front of noise_r)
        if (mv == nullptr) return;
        const int64_t k = mv->n_moves;
        TORCH_CHECK(mv->noise_g.has_value() == mv->noise_h.has_value(), "fabhip: pass both noise_g and noise_h or neither");
        mv->g = mv->noise_g.has_value() ? *mv->noise_g : at::randn({M, k, B, dim}, eps0.options());
        mv->h = mv->noise_h.has_value() ? *mv->noise_h : at::empty({M, k, B}, eps0.options()).exponential_(1.0);
        mv->p_accept = fempty({M, k}, eps0);
        fm.noise_g = fpn(mv->g, M * k * B * dim, eps0, "noise_g"); fm.noise_h = fpn(mv->h, M * k * B, eps0, "noise_h");
        fm.p_accept_out = mv->p_accept.data_ptr<float>();
    };
    const fabhip_stream_t st = stream_of(eps0);
    // defensive mixture: `sel` absent: drawn after eps0 (the caller's draw) and before the transition noise
    Tensor sel;
    if (mix != nullptr) {
        ma = make_mix(*mix, dim, eps0);
        if (mix->enabled) {
            sel = mix->sel.has_value() ? *mix->sel : at::rand({B}, eps0.options());
            ma.sel = fpn(sel, B, eps0, "sel");
        }
    }
    const bool named = ext != nullptr;
    if (!draw_inside) {
        moves_noise();
        smc_outputs();
        chk(fabhip_ais_run_ext(&a, xp, st), named ? "ais_run_ext" : "ais_run");
    } else {
        chk(fabhip_ais_phase_ext(&a, xp, FABHIP_AIS_INIT, 1, 0, nullptr, st),      // (reads no noise of the transitions or moves)
            named ? "ais_run_ext (chain initialisation)" : "ais_run (chain initialisation)");
        noise_a = at::randn({M, n_inner, B, dim}, eps0.options());
        noise_b = hmc ? at::empty({M, n_inner, B}, eps0.options()).exponential_(1.0) : at::rand({M, n_inner, B}, eps0.options());
        a.noise_a = noise_a.data_ptr<float>(); a.noise_b = noise_b.data_ptr<float>();
        moves_noise();
        smc_outputs();
        chk(fabhip_ais_phase_ext(&a, xp, FABHIP_AIS_CONTINUE | FABHIP_AIS_FINISH, 1, (int32_t)M, nullptr, st),
            named ? "ais_run_ext (transitions)" : "ais_run (transitions)");
    }
    return {x, lq, lp, gq, gp, log_w, o.n_valid, o.stats, o.base_x, o.base_lw};
}

// The headline op: the whole call without any optional mode.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> ais_run(
    const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t kind, at::ArrayRef<double> prm,
    const optional<Tensor>& locs, const optional<Tensor>& scales, at::ArrayRef<double> betas, double alpha,
    bool p_target, int64_t transition, const Tensor& eps0, const optional<Tensor>& noise_a, const optional<Tensor>& noise_b,
    Tensor step_state, optional<Tensor> common_epsilon, const optional<Tensor>& mass, int64_t n_inner, int64_t L, double max_grad,
    double target_p_accept, bool tune, optional<Tensor> p_accept_first, optional<Tensor> p_accept_last,
    optional<Tensor> avg_distance_first, optional<Tensor> avg_distance_last, bool want_base, int64_t precision) {
    return ais_run_impl(nullptr, packed, dim, n_layers, width, kind, prm, locs, scales, betas, alpha, p_target, transition, eps0,
                        noise_a, noise_b, step_state, common_epsilon, mass, n_inner, L, max_grad, target_p_accept, tune,
                        p_accept_first, p_accept_last, avg_distance_first, avg_distance_last, want_base, precision);
}

// The five outputs the modes add behind the ten of ais_run: resampled int32[M], ess float[M], ancestors int32[M, B], log_w_pre
// float[M, B] (SMC mode; the last two only with want_trace), the moves' acceptance fractions float[M, n_moves].  Empty where the
// mode is off.
static void push_ext_outputs(std::vector<Tensor>& out, const AisExtOp& ext, const Tensor& like) {
    auto e = [&](const Tensor& v, at::ScalarType ty) { return v.defined() ? v : at::empty({0}, like.options().dtype(ty)); };
    const SmcOp smc = ext.smc.value_or(SmcOp{});
    out.push_back(e(smc.resampled, at::kInt)); out.push_back(e(smc.ess, at::kFloat));
    out.push_back(e(smc.ancestors, at::kInt)); out.push_back(e(smc.log_w_pre, at::kFloat));
    out.push_back(e(ext.moves.has_value() ? ext.moves->p_accept : Tensor(), at::kFloat));
}

// ais_run with its optional modes, each named by its parameter group (fabhip_ais_run_ext): SMC mode (`tau` given), the defensive
// mixture as base distribution (`mix_loc` given; mix_enabled = false: the call without it through the same entry points), n_moves
// > 0 flow-proposal moves in front of every transition.  Fifteen outputs, always: ais_run's ten, then push_ext_outputs' five.
std::vector<Tensor> ais_run_ext(
    const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t kind, at::ArrayRef<double> prm,
    const optional<Tensor>& locs, const optional<Tensor>& scales, at::ArrayRef<double> betas, double alpha,
    bool p_target, int64_t transition, const Tensor& eps0, const optional<Tensor>& noise_a, const optional<Tensor>& noise_b,
    Tensor step_state, optional<Tensor> common_epsilon, const optional<Tensor>& mass, int64_t n_inner, int64_t L, double max_grad,
    double target_p_accept, bool tune, optional<Tensor> p_accept_first, optional<Tensor> p_accept_last,
    optional<Tensor> avg_distance_first, optional<Tensor> avg_distance_last, bool want_base, int64_t precision,
    optional<double> tau, const optional<Tensor>& noise_r, bool want_trace, int64_t method, const optional<Tensor>& mix_loc,
    const optional<Tensor>& mix_log_scale, const optional<Tensor>& mix_logit, const optional<Tensor>& sel, bool mix_enabled,
    int64_t n_moves, const optional<Tensor>& noise_g, const optional<Tensor>& noise_h) {
    AisExtOp ext;
    if (tau.has_value()) ext.smc = SmcOp{*tau, noise_r, want_trace, method};
    TORCH_CHECK(mix_loc.has_value() == mix_log_scale.has_value() && mix_loc.has_value() == mix_logit.has_value(),
                "fabhip: pass mix_loc, mix_log_scale and mix_logit together or none of them");
    if (mix_loc.has_value()) ext.mix = MixOp{mix_enabled, *mix_loc, *mix_log_scale, *mix_logit, sel};
    TORCH_CHECK(n_moves >= 0, "fabhip: n_moves must be >= 0");
    if (n_moves > 0) ext.moves = MovesOp{n_moves, noise_g, noise_h};
    std::vector<Tensor> out = std::apply(
        [](auto&&... t) { return std::vector<Tensor>{t...}; },
        ais_run_impl(&ext, packed, dim, n_layers, width, kind, prm, locs, scales, betas, alpha, p_target, transition, eps0, noise_a,
                     noise_b, step_state, common_epsilon, mass, n_inner, L, max_grad, target_p_accept, tune, p_accept_first,
                     p_accept_last, avg_distance_first, avg_distance_last, want_base, precision));
    push_ext_outputs(out, ext, eps0);
    return out;
}

// One flow-proposal independence move on Point tensors, in place (fabhip_flow_move): (acceptance fraction float[1], accepted
// rows int32[1]).  grad_log_q / grad_log_p absent: a gradient-free operator's point.  n_valid (int32, device): rows in use.
std::tuple<Tensor, Tensor> flow_move(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t kind,
                                     at::ArrayRef<double> prm, const optional<Tensor>& locs, const optional<Tensor>& scales, Tensor x,
                                     Tensor log_q, Tensor log_p, optional<Tensor> grad_log_q, optional<Tensor> grad_log_p,
                                     const optional<Tensor>& n_valid, double beta, double alpha, bool p_target,
                                     const Tensor& noise_g, const Tensor& noise_h, int64_t precision) {
    c10::DeviceGuard g(x.device());
    fabhip_flow_move_args a = {};
    a.flow = make_flow(packed, dim, n_layers, width, precision);
    a.target = make_target(kind, prm, locs, scales, dim, packed);
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [B, dim]");
    TORCH_CHECK(grad_log_q.has_value() == grad_log_p.has_value(), "fabhip: pass both gradient fields of the Point or neither");
    const int64_t B = x.size(0);
    const bool wg = grad_log_q.has_value();
    a.point = fabhip_point{fpm(x, "x"), fpmn(log_q, B, x, "log_q"), fpmn(log_p, B, x, "log_p"),
                           wg ? fpmn(*grad_log_q, B * dim, x, "grad_log_q") : nullptr,
                           wg ? fpmn(*grad_log_p, B * dim, x, "grad_log_p") : nullptr};
    a.B = B;
    if (n_valid.has_value()) {
        need(*n_valid, at::kInt, "n_valid"); need_n(*n_valid, 1, x, "n_valid", true);
        a.n_valid = n_valid->data_ptr<int32_t>();
    }
    a.cur = coefs(beta, alpha, p_target);
    a.noise_g = fpn(noise_g, B * dim, x, "noise_g"); a.noise_h = fpn(noise_h, B, x, "noise_h");
    Tensor frac = fempty({1}, x), count = at::empty({1}, x.options().dtype(at::kInt));
    a.p_accept = frac.data_ptr<float>(); a.n_accept = count.data_ptr<int32_t>();
    const size_t nb = fabhip_flow_move_workspace_bytes(B, (int32_t)dim);
    Tensor ws = scratch(nb, x);
    a.workspace = aligned(ws); a.workspace_bytes = nb;
    chk(fabhip_flow_move(&a, stream_of(x)), "flow_move");
    return {frac, count};
}

// The mixture's density (and d/dx with with_grad) at x [B, dim]: one launch (fabhip_defensive_log_prob).
std::tuple<Tensor, Tensor> defensive_log_prob(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, const Tensor& loc,
                                              const Tensor& log_scale, const Tensor& logit, const Tensor& x, bool with_grad,
                                              int64_t precision) {
    c10::DeviceGuard g(x.device());
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [B, dim]");
    const fabhip_flow f = make_flow(packed, dim, n_layers, width, precision);
    need_n(packed, packed.numel(), x, "packed flow image");
    MixOp mix;
    mix.loc = loc; mix.log_scale = log_scale; mix.logit = logit;
    const fabhip_defensive_args ma = make_mix(mix, dim, x);
    const int64_t B = x.size(0);
    Tensor lq = fempty({B}, x), gx = with_grad ? fempty({B, dim}, x) : fempty({0}, x);
    chk(fabhip_defensive_log_prob(&f, &ma, fp(x, "x"), lq.data_ptr<float>(), with_grad ? gx.data_ptr<float>() : nullptr, B,
                                  nullptr, stream_of(x)),
        "defensive_log_prob");
    return {lq, gx};
}

// The same call in pieces (fabhip_ais_phase): the state tensors are the caller's, in/out across the phases of one AIS
// run.  `ais_phase_args` fills the call's arguments and returns the checked slab pointer (`partials`: the acceptance sums of a
// deferred adaptation); the ops below decide what to run on them.
float* ais_phase_args(AisCall& c, const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t kind,
                      at::ArrayRef<double> prm, const optional<Tensor>& locs, const optional<Tensor>& scales,
                      at::ArrayRef<double> betas, double alpha, bool p_target, int64_t transition, const optional<Tensor>& eps0,
                      const Tensor& noise_a, const Tensor& noise_b, const Tensor& step_state,
                      const optional<Tensor>& common_epsilon, const optional<Tensor>& mass, int64_t n_inner, int64_t L,
                      double max_grad, double target_p_accept, bool tune, const Tensor& x, const Tensor& log_q,
                      const Tensor& log_p, const optional<Tensor>& grad_log_q, const optional<Tensor>& grad_log_p,
                      const Tensor& log_w, const Tensor& n_valid, const Tensor& stats, const optional<Tensor>& partials,
                      const optional<Tensor>& p_accept_first, const optional<Tensor>& p_accept_last,
                      const optional<Tensor>& avg_distance_first, const optional<Tensor>& avg_distance_last,
                      const optional<Tensor>& base_x, const optional<Tensor>& base_log_w, int64_t precision,
                      const fabhip_ais_ext* ext) {
    TORCH_CHECK(x.dim() == 2 && x.size(1) == dim, "fabhip: x must be [B, dim]");
    fill_ais_args(c, packed, dim, n_layers, width, kind, prm, locs, scales, betas, alpha, p_target, transition, x.size(0), x,
                  step_state, common_epsilon, mass, n_inner, L, max_grad, target_p_accept, tune, p_accept_first, p_accept_last,
                  avg_distance_first, avg_distance_last, precision, ext);
    fabhip_ais_args& a = c.a;
    const int64_t B = c.B, M = c.M;
    TORCH_CHECK(!c.hmc || (grad_log_q.has_value() && grad_log_p.has_value()),
                "fabhip: an HMC AIS run needs the gradient fields of the Point");
    a.eps0 = eps0.has_value() ? fpn(*eps0, B * dim, x, "eps0") : nullptr;
    a.noise_a = fpn(noise_a, M * n_inner * B * dim, x, "noise_a"); a.noise_b = fpn(noise_b, M * n_inner * B, x, "noise_b");
    a.point = fabhip_point{fpm(x, "x"), fpmn(log_q, B, x, "log_q"), fpmn(log_p, B, x, "log_p"),
                           c.hmc ? fpmn(*grad_log_q, B * dim, x, "grad_log_q") : nullptr,
                           c.hmc ? fpmn(*grad_log_p, B * dim, x, "grad_log_p") : nullptr};
    a.log_w = fpmn(log_w, B, x, "log_w");
    need(n_valid, at::kInt, "n_valid"); need_n(n_valid, 2, x, "n_valid");
    a.n_valid = n_valid.data_ptr<int32_t>();
    a.stats = fpmn(stats, 16, x, "stats");
    a.base_x = fpmn_opt(base_x, B * dim, x, "base_x");
    a.base_log_w = fpmn_opt(base_log_w, B, x, "base_log_w");
    return fpmn_opt(partials, c.hmc ? fabhip_hmc_partials_floats(B)
                                    : fabhip_metropolis_partials_floats(B, (int32_t)M, (int32_t)n_inner), x, "partials");
}

// ais_phase: the phases and transitions the caller names, once (fabhip_ais_phase_ext with a NULL fabhip_ais_ext).
void ais_phase(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t kind, at::ArrayRef<double> prm,
               const optional<Tensor>& locs, const optional<Tensor>& scales, at::ArrayRef<double> betas, double alpha, bool p_target,
               int64_t transition, int64_t phases, int64_t j_begin, int64_t j_end, const optional<Tensor>& eps0,
               const Tensor& noise_a, const Tensor& noise_b, Tensor step_state, optional<Tensor> common_epsilon,
               const optional<Tensor>& mass, int64_t n_inner, int64_t L, double max_grad, double target_p_accept, bool tune, Tensor x,
               Tensor log_q, Tensor log_p, optional<Tensor> grad_log_q, optional<Tensor> grad_log_p, Tensor log_w, Tensor n_valid,
               Tensor stats, optional<Tensor> partials, optional<Tensor> p_accept_first, optional<Tensor> p_accept_last,
               optional<Tensor> avg_distance_first, optional<Tensor> avg_distance_last, optional<Tensor> base_x,
               optional<Tensor> base_log_w, int64_t precision) {
    c10::DeviceGuard g(x.device());
    AisCall c;
    float* slab = ais_phase_args(c, packed, dim, n_layers, width, kind, prm, locs, scales, betas, alpha, p_target, transition, eps0,
                                 noise_a, noise_b, step_state, common_epsilon, mass, n_inner, L, max_grad, target_p_accept, tune,
                                 x, log_q, log_p, grad_log_q, grad_log_p, log_w, n_valid, stats, partials, p_accept_first,
                                 p_accept_last, avg_distance_first, avg_distance_last, base_x, base_log_w, precision, nullptr);
    chk(fabhip_ais_phase_ext(&c.a, nullptr, (int32_t)phases, (int32_t)j_begin, (int32_t)j_end, slab, stream_of(x)), "ais_phase");
}

// ais_phase with the SMC mode: transition j's phase starts with its resampling step (`only_resample`: and ends there).  The
// records are the caller's, [M] / [M, B]; only the rows of the transitions this call runs are written.
void ais_phase_smc(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t kind, at::ArrayRef<double> prm,
                   const optional<Tensor>& locs, const optional<Tensor>& scales, at::ArrayRef<double> betas, double alpha,
                   bool p_target, int64_t transition, int64_t phases, int64_t j_begin, int64_t j_end,
                   const optional<Tensor>& eps0, const Tensor& noise_a, const Tensor& noise_b, Tensor step_state,
                   optional<Tensor> common_epsilon, const optional<Tensor>& mass, int64_t n_inner, int64_t L, double max_grad,
                   double target_p_accept, bool tune, Tensor x, Tensor log_q, Tensor log_p, optional<Tensor> grad_log_q,
                   optional<Tensor> grad_log_p, Tensor log_w, Tensor n_valid, Tensor stats, optional<Tensor> partials,
                   optional<Tensor> p_accept_first, optional<Tensor> p_accept_last, optional<Tensor> avg_distance_first,
                   optional<Tensor> avg_distance_last, optional<Tensor> base_x, optional<Tensor> base_log_w, int64_t precision,
                   optional<double> tau, const optional<Tensor>& noise_r, bool only_resample, optional<Tensor> resampled,
                   optional<Tensor> ess, optional<Tensor> ancestors, optional<Tensor> log_w_pre, int64_t method) {
    const int64_t B = x.size(0), M = (int64_t)betas.size() - 2;
    fabhip_smc_args sa = {};
    sa.enabled = tau.has_value() ? 1 : 0; sa.only_resample = only_resample ? 1 : 0; sa.tau = tau.has_value() ? *tau : 0.0;
    sa.method = (int32_t)method;
    if (sa.enabled) {
        TORCH_CHECK(noise_r.has_value(), "fabhip: ais_phase_smc needs noise_r (float64 [M]) when tau is given");
        sa.u = smc_uniforms(noise_r, M, x).data_ptr<double>();
        auto ints = [&](optional<Tensor>& t, int64_t n, const char* what) -> int32_t* {
            if (!t.has_value()) return nullptr;
            need(*t, at::kInt, what); need_n(*t, n, x, what);
            return t->data_ptr<int32_t>();
        };
        sa.resampled = ints(resampled, M, "resampled");
        sa.ancestors = ints(ancestors, M * B, "ancestors");
        sa.ess = fpmn_opt(ess, M, x, "ess");
        sa.log_w_pre = fpmn_opt(log_w_pre, M * B, x, "log_w_pre");
    }
    c10::DeviceGuard g(x.device());
    const fabhip_ais_ext ext = {&sa, nullptr, nullptr};
    AisCall c;
    float* slab = ais_phase_args(c, packed, dim, n_layers, width, kind, prm, locs, scales, betas, alpha, p_target, transition, eps0,
                                 noise_a, noise_b, step_state, common_epsilon, mass, n_inner, L, max_grad, target_p_accept, tune,
                                 x, log_q, log_p, grad_log_q, grad_log_p, log_w, n_valid, stats, partials, p_accept_first,
                                 p_accept_last, avg_distance_first, avg_distance_last, base_x, base_log_w, precision, &ext);
    chk(fabhip_ais_phase_ext(&c.a, &ext, (int32_t)phases, (int32_t)j_begin, (int32_t)j_end, slab, stream_of(x)), "ais_phase_smc");
}

// The decision of the SMC step alone (fabhip_smc_decide) for samplers that step their transitions from Python:
// (ancestors int64[n] - gather_rows takes them as they are -, resampled int32[1], ess float[1], log_w_common float[1]).
// `method`: FABHIP_SMC_SYSTEMATIC (0) or FABHIP_SMC_STRATIFIED (1: the seed is the 64 bits of u).
std::tuple<Tensor, Tensor, Tensor, Tensor> smc_decide(const Tensor& log_w, double tau, const Tensor& u, int64_t method) {
    c10::DeviceGuard g(log_w.device());
    const int64_t n = log_w.numel();
    TORCH_CHECK(n >= 1, "fabhip: smc_decide needs at least one chain");
    need(u, at::kDouble, "u");
    TORCH_CHECK(u.numel() == 1 && u.device() == log_w.device(), "fabhip: u must be ONE float64 on log_w's device");
    Tensor anc = at::empty({n}, log_w.options().dtype(at::kInt)), flag = at::empty({1}, log_w.options().dtype(at::kInt));
    Tensor ess = fempty({1}, log_w), common = fempty({1}, log_w);
    const size_t nb = fabhip_smc_workspace_bytes(n);
    Tensor ws = scratch(nb, log_w);
    chk(fabhip_smc_decide(fp(log_w, "log_w"), n, nullptr, tau, u.data_ptr<double>(), anc.data_ptr<int32_t>(),
                          flag.data_ptr<int32_t>(), ess.data_ptr<float>(), common.data_ptr<float>(), nullptr, aligned(ws), nb,
                          (int32_t)method, stream_of(log_w)),
        "smc_decide");
    return {anc.to(at::kLong), flag, ess, common};
}

// The next temperature of an adaptive schedule (fabhip_next_beta): float64 [4] = beta_next, ess0, ESS at the choice,
// evaluations + 2^16 floor.  The output is the op's own tensor and nothing else is written: a call made in pieces keeps the
// state FABHIP_AIS_INIT left in its workspace.
Tensor next_beta(const Tensor& log_w, const Tensor& log_q, const Tensor& log_p, const optional<Tensor>& n_valid, double beta,
                 double alpha, bool p_target, double rho, int64_t iters) {
    c10::DeviceGuard g(log_w.device());
    const int64_t n = log_w.numel();
    TORCH_CHECK(n >= 1, "fabhip: next_beta needs at least one chain");
    need_n(log_q, n, log_w, "log_q"); need_n(log_p, n, log_w, "log_p");
    const int32_t* np = nullptr;
    if (n_valid.has_value()) {
        need(*n_valid, at::kInt, "n_valid");
        TORCH_CHECK(n_valid->numel() >= 1 && n_valid->device() == log_w.device(), "fabhip: n_valid must be int32 on log_w's device");
        np = n_valid->data_ptr<int32_t>();
    }
    Tensor out = at::empty({4}, log_w.options().dtype(at::kDouble));
    chk(fabhip_next_beta(fp(log_w, "log_w"), fp(log_q, "log_q"), fp(log_p, "log_p"), n, np, beta, alpha, p_target ? 1 : 0, rho,
                         (int32_t)iters, out.data_ptr<double>(), stream_of(log_w)),
        "next_beta");
    return out;
}

// SMC mode over sharded chains (fabhip_smc_shard_pack / fabhip_smc_shard_resample; fab_torch_amd/parallel.py steps the loop).
// pack: this rank's send buffer [b + 1, 3 D + 4] (row b: its live count, read from n_valid on the device).
static fabhip_point shard_point(const Tensor& x, const Tensor& log_q, const Tensor& log_p, const optional<Tensor>& gq,
                                const optional<Tensor>& gp) {
    TORCH_CHECK(x.dim() == 2 && x.size(0) >= 1, "fabhip: x must be [b, D] with b >= 1");
    TORCH_CHECK(gq.has_value() == gp.has_value(), "fabhip: grad_log_q and grad_log_p come together");
    const int64_t b = x.size(0), D = x.size(1);
    return fabhip_point{fpm(x, "x"), fpmn(log_q, b, x, "log_q"), fpmn(log_p, b, x, "log_p"),
                        fpmn_opt(gq, b * D, x, "grad_log_q"), fpmn_opt(gp, b * D, x, "grad_log_p")};
}

Tensor smc_shard_pack(const Tensor& x, const Tensor& log_q, const Tensor& log_p, const optional<Tensor>& grad_log_q,
                      const optional<Tensor>& grad_log_p, const Tensor& log_w, const Tensor& n_valid) {
    c10::DeviceGuard g(x.device());
    const fabhip_point pt = shard_point(x, log_q, log_p, grad_log_q, grad_log_p);
    const int64_t b = x.size(0), D = x.size(1);
    need(n_valid, at::kInt, "n_valid"); need_n(n_valid, 1, x, "n_valid", true);
    Tensor send = fempty({b + 1, 3 * D + 4}, x);
    chk(fabhip_smc_shard_pack(&pt, fpn(log_w, b, x, "log_w"), n_valid.data_ptr<int32_t>(), b, (int32_t)D,
                              send.data_ptr<float>(), stream_of(x)), "smc_shard_pack");
    return send;
}

// resample: the state tensors in place; (resampled int32[1], ess float[1], ancestors int32[R b], log_w_pre float[R b]) - the
// last two empty unless want_trace.
std::tuple<Tensor, Tensor, Tensor, Tensor> smc_shard_resample(
    const Tensor& gathered, int64_t world, int64_t rank, double tau, const Tensor& u, Tensor x, Tensor log_q, Tensor log_p,
    optional<Tensor> grad_log_q, optional<Tensor> grad_log_p, Tensor log_w, const Tensor& n_valid, bool want_trace) {
    c10::DeviceGuard g(x.device());
    const fabhip_point pt = shard_point(x, log_q, log_p, grad_log_q, grad_log_p);
    const int64_t b = x.size(0), D = x.size(1);
    TORCH_CHECK(world >= 1 && rank >= 0 && rank < world, "fabhip: smc_shard_resample needs 0 <= rank < world");
    need(u, at::kDouble, "u");
    TORCH_CHECK(u.numel() == 1 && u.device() == x.device(), "fabhip: u must be ONE float64 on the state's device");
    need(n_valid, at::kInt, "n_valid"); need_n(n_valid, 1, x, "n_valid", true);
    const float* gat = fpn(gathered, world * (b + 1) * (3 * D + 4), x, "gathered");
    Tensor flag = at::empty({1}, x.options().dtype(at::kInt)), ess = fempty({1}, x);
    Tensor anc = at::empty({want_trace ? world * b : 0}, x.options().dtype(at::kInt));
    Tensor pre = fempty({want_trace ? world * b : 0}, x);
    const size_t nb = fabhip_smc_shard_workspace_bytes((int32_t)world, b);
    Tensor ws = scratch(nb, x);
    chk(fabhip_smc_shard_resample(gat, (int32_t)world, (int32_t)rank, b, (int32_t)D, tau, u.data_ptr<double>(), &pt,
                                  fpmn(log_w, b, x, "log_w"), n_valid.data_ptr<int32_t>(), flag.data_ptr<int32_t>(),
                                  ess.data_ptr<float>(), want_trace ? anc.data_ptr<int32_t>() : nullptr,
                                  want_trace ? pre.data_ptr<float>() : nullptr, aligned(ws), nb, stream_of(x)),
        "smc_shard_resample");
    return {flag, ess, anc, pre};
}

// One shard's WHOLE tuned AIS call in one op: chain initialisation, M x {HMC transition publishing its
// acceptance slab, ONE all-gather of the slabs through the c10d process group registered as `group_name` (RCCL over xGMI
// on a GPU node), the step-size rule of hmc.py:162-170 on the joined slabs in rank order (fabhip_hmc_adapt_gathered: every
// rank applies it to the same numbers)}, "chain end" filter + this shard's ESS / log Z.  Same kernels, same order and the
// same values as fab_torch_amd/parallel.py's Python-stepped loop (kept as the reference implementation the tests compare
// with); what goes is 2 M + 1 dispatcher round trips and M Python-level collectives per call.  Returns the collectives issued.
int64_t ais_sharded_tuned(const Tensor& packed, int64_t dim, int64_t n_layers, int64_t width, int64_t kind,
                          at::ArrayRef<double> prm, const optional<Tensor>& locs, const optional<Tensor>& scales,
                          at::ArrayRef<double> betas, double alpha, bool p_target, int64_t transition,
                          const optional<Tensor>& eps0, const Tensor& noise_a, const Tensor& noise_b, Tensor step_state,
                          optional<Tensor> common_epsilon, const optional<Tensor>& mass, int64_t L, double max_grad,
                          double target_p_accept, Tensor x, Tensor log_q, Tensor log_p, optional<Tensor> grad_log_q,
                          optional<Tensor> grad_log_p, Tensor log_w, Tensor n_valid, Tensor stats, Tensor partials,
                          optional<Tensor> p_accept_first, optional<Tensor> p_accept_last,
                          optional<Tensor> avg_distance_first, optional<Tensor> avg_distance_last, int64_t precision,
                          std::string group_name) {
    c10::DeviceGuard g(x.device());
    AisCall c;
    float* slab = ais_phase_args(c, packed, dim, n_layers, width, kind, prm, locs, scales, betas, alpha, p_target, transition, eps0,
                                 noise_a, noise_b, step_state, common_epsilon, mass, 1, L, max_grad, target_p_accept, true, x,
                                 log_q, log_p, grad_log_q, grad_log_p, log_w, n_valid, stats, partials, p_accept_first,
                                 p_accept_last, avg_distance_first, avg_distance_last, c10::nullopt, c10::nullopt, precision, nullptr);
    const fabhip_ais_args& a = c.a;
    const int64_t B = c.B, M = c.M;
    TORCH_CHECK(c.hmc, "fabhip: ais_sharded_tuned is HMC with n_outer == 1 (the acceptance slab: hmc_partials_floats(B) floats)");
    auto pg = c10d::resolve_process_group(group_name);
    const int64_t world = pg->getSize(), nslab = fabhip_hmc_partials_floats(B);
    // RCCL ("nccl") takes the device slab as it is: the collective is ordered behind the transition on the current stream
    // and Work::wait() orders the stream behind the collective - the host never blocks.  A host-only backend (gloo: the
    // CPU-side tests of the N > 1 path, two ranks on a one-GPU box) is fed through the host.
    bool device_collective = false;
    try {
        device_collective = pg->getBackend(c10::DeviceType::CUDA)->getBackendName() == "nccl";
    } catch (const std::exception&) {                     // no backend registered for device tensors: through the host
    }
    Tensor gathered = fempty({world * nslab}, x), host_in, host_out;
    if (!device_collective) {
        host_in = at::empty({nslab}, at::TensorOptions().dtype(at::kFloat).device(at::kCPU));
        host_out = at::empty({world * nslab}, host_in.options());
    }
    const fabhip_stream_t st = stream_of(x);
    chk(fabhip_ais_phase(&a, FABHIP_AIS_INIT, 1, 0, nullptr, st), "ais_sharded_tuned (chain initialisation)");
    int64_t n_collectives = 0;
    for (int64_t j = 1; j <= M; ++j) {
        chk(fabhip_ais_phase(&a, 0, (int32_t)j, (int32_t)j, slab, st), "ais_sharded_tuned (transition)");
        if (world > 1 || device_collective) {          // (a one-rank RCCL group still runs the collective: the path a node takes)
            if (device_collective) {
                pg->_allgather_base(gathered, partials)->wait();
            } else {
                host_in.copy_(partials);
                pg->_allgather_base(host_out, host_in)->wait();
                gathered.copy_(host_out);
            }
            ++n_collectives;
        } else {
            gathered.copy_(partials);
        }
        float* pa = j == 1 ? a.p_accept_first : (j == M ? a.p_accept_last : nullptr);        // hmc.py:173-183 (store_info)
        float* ad = j == 1 ? a.avg_distance_first : (j == M ? a.avg_distance_last : nullptr);
        chk(fabhip_hmc_adapt_gathered(gathered.data_ptr<float>(), (int32_t)world, B, a.step_state + (j - 1), a.common_epsilon,
                                      a.target_p_accept, 1, pa, ad, st),
            "ais_sharded_tuned (step-size rule on the gathered slabs)");
    }
    chk(fabhip_ais_phase(&a, FABHIP_AIS_FINISH, 1, 0, nullptr, st), "ais_sharded_tuned (chain end)");
    return n_collectives;
}

// Linear backward over a tape (fabhip_tape_gemm): Y / X are views INTO `tape` given as float offsets of layer 0
std::tuple<Tensor, Tensor> tape_gemm(const Tensor& tape, int64_t layer_stride, int64_t L, int64_t off_y, int64_t ldy, int64_t P,
                                     int64_t off_x, int64_t ldx, int64_t Q, const Tensor& coef, bool want_colsum) {
    c10::DeviceGuard g(tape.device());
    const int64_t B = coef.numel();
    TORCH_CHECK(L >= 1 && P >= 1 && Q >= 1 && ldy >= P && ldx >= Q && off_y >= 0 && off_x >= 0, "fabhip: tape_gemm shapes");
    TORCH_CHECK((L - 1) * layer_stride + off_y + B * ldy <= tape.numel() && (L - 1) * layer_stride + off_x + B * ldx <= tape.numel(),
                "fabhip: tape_gemm operands leave the tape");
    need_n(coef, B, tape, "coef");
    Tensor C = fempty({L, P, Q}, tape), S = want_colsum ? fempty({L, P}, tape) : fempty({0}, tape);
    const float* t = fp(tape, "tape");
    chk(fabhip_tape_gemm(t + off_y, layer_stride, (int32_t)ldy, (int32_t)P, t + off_x, layer_stride, (int32_t)ldx, (int32_t)Q,
                         fp(coef, "coef"), B, (int32_t)L, C.data_ptr<float>(), want_colsum ? S.data_ptr<float>() : nullptr,
                         stream_of(tape)),
        "tape_gemm");
    return {C, S};
}

int64_t hmc_partials_floats(int64_t B) { return fabhip_hmc_partials_floats(B); }
int64_t metropolis_partials_floats(int64_t B, int64_t M, int64_t n_updates) {
    return fabhip_metropolis_partials_floats(B, (int32_t)M, (int32_t)n_updates);
}

// metropolis.py:68-73 on the acceptance of ALL chains of a sharded batch, for the M transitions of one AIS call at once
void metropolis_adapt_gathered(const Tensor& gathered, int64_t n_ranks, int64_t B_rank, Tensor noise_scalings,
                               double target_p_accept, bool tune) {
    c10::DeviceGuard g(gathered.device());
    TORCH_CHECK(n_ranks >= 1 && B_rank >= 1 && noise_scalings.dim() == 2, "fabhip: metropolis_adapt_gathered needs n_ranks, "
                "B_rank >= 1 and noise_scalings [M, n_updates]");
    const int64_t M = noise_scalings.size(0), nu = noise_scalings.size(1);
    need_n(gathered, n_ranks * fabhip_metropolis_partials_floats(B_rank, (int32_t)M, (int32_t)nu), gathered, "gathered partials");
    chk(fabhip_metropolis_adapt_gathered(fp(gathered, "gathered partials"), (int32_t)n_ranks, B_rank, (int32_t)M, (int32_t)nu,
                                         fpmn(noise_scalings, M * nu, gathered, "noise_scalings"), (float)target_p_accept,
                                         tune ? 1 : 0, stream_of(gathered)),
        "metropolis_adapt_gathered");
}

void hmc_adapt_gathered(const Tensor& gathered, int64_t n_ranks, int64_t B_rank, Tensor epsilon, Tensor common_epsilon,
                        double target_p_accept, bool tune, optional<Tensor> p_accept, optional<Tensor> avg_distance) {
    c10::DeviceGuard g(gathered.device());
    TORCH_CHECK(n_ranks >= 1 && B_rank >= 1, "fabhip: hmc_adapt_gathered needs n_ranks, B_rank >= 1");
    need_n(gathered, n_ranks * fabhip_hmc_partials_floats(B_rank), gathered, "gathered partials");
    chk(fabhip_hmc_adapt_gathered(fp(gathered, "gathered partials"), (int32_t)n_ranks, B_rank,
                                  fpmn(epsilon, 1, gathered, "epsilon"), fpmn(common_epsilon, 1, gathered, "common_epsilon", true),
                                  (float)target_p_accept, tune ? 1 : 0, fpmn_opt(p_accept, 1, gathered, "p_accept", true),
                                  fpmn_opt(avg_distance, 1, gathered, "avg_distance", true), stream_of(gathered)),
        "hmc_adapt_gathered");
}

// ------------------------------------------------------------------------------------------------------------------
// ESS / log Z, resampling, top-k
// ------------------------------------------------------------------------------------------------------------------
Tensor ess_logz(const Tensor& log_w, const optional<Tensor>& n_ptr, double n_norm) {
    c10::DeviceGuard g(log_w.device());
    const int64_t n = log_w.numel();
    Tensor out = fempty({3}, log_w);
    const size_t nb = fabhip_ess_workspace_bytes(n);
    Tensor ws = scratch(nb, log_w);
    const int32_t* np = nullptr;
    if (n_ptr.has_value()) { need(*n_ptr, at::kInt, "n_ptr"); np = n_ptr->data_ptr<int32_t>(); }
    chk(fabhip_ess_logz(fp(log_w, "log_w"), n, np, n_norm, out.data_ptr<float>(), aligned(ws), nb, stream_of(log_w)),
        "ess_logz");
    return out;
}

Tensor resample_multinomial(const Tensor& log_w, const Tensor& u) {
    c10::DeviceGuard g(log_w.device());
    need(u, at::kDouble, "u");
    const int64_t n = log_w.numel(), ns = u.numel();
    Tensor idx = at::empty({ns}, log_w.options().dtype(at::kLong));
    const size_t nb = fabhip_resample_workspace_bytes(n);
    Tensor ws = scratch(nb, log_w);
    chk(fabhip_resample_multinomial(fp(log_w, "log_w"), n, u.data_ptr<double>(), ns, idx.data_ptr<int64_t>(),
                                    aligned(ws), nb, stream_of(log_w)),
        "resample_multinomial");
    return idx;
}

// scan pass alone (after a first full call): returns the workspace so that a caller can time repeated scans
Tensor fixed_cdf(const Tensor& log_w, optional<Tensor> workspace) {
    c10::DeviceGuard g(log_w.device());
    const int64_t n = log_w.numel();
    const size_t nb = fabhip_resample_workspace_bytes(n);
    Tensor ws = workspace.has_value() ? *workspace : scratch(nb, log_w);
    chk(fabhip_fixed_cdf(fp(log_w, "log_w"), n, workspace.has_value() ? 1 : 0, nullptr, aligned(ws), nb, stream_of(log_w)),
        "fixed_cdf");
    return ws;
}

Tensor resample_systematic(const Tensor& log_w, double u0, int64_t n_samples) {
    c10::DeviceGuard g(log_w.device());
    const int64_t n = log_w.numel();
    Tensor idx = at::empty({n_samples}, log_w.options().dtype(at::kLong));
    const size_t nb = fabhip_resample_workspace_bytes(n);
    Tensor ws = scratch(nb, log_w);
    chk(fabhip_resample_systematic(fp(log_w, "log_w"), n, u0, n_samples, idx.data_ptr<int64_t>(), aligned(ws), nb,
                                   stream_of(log_w)),
        "resample_systematic");
    return idx;
}

// The seeded resamplers (one C signature): int64 [n_samples] indices; the 64 bits of `seed` are the C ABI's uint64 seed
// (order: FABHIP_ORDER_*)
using SeededSizeFn = size_t (*)(int64_t, int64_t);
using SeededFn = int (*)(const float*, int64_t, uint64_t, int64_t, int32_t, int64_t*, void*, size_t, fabhip_stream_t);
static Tensor resample_seeded(SeededSizeFn size_fn, SeededFn fn, const char* name, const Tensor& log_w, int64_t seed,
                              int64_t n_samples, int64_t order) {
    c10::DeviceGuard g(log_w.device());
    const int64_t n = log_w.numel();
    TORCH_CHECK(n_samples >= 1, "fabhip::", name, ": n_samples must be >= 1");
    Tensor idx = at::empty({n_samples}, log_w.options().dtype(at::kLong));
    const size_t nb = size_fn(n, n_samples);
    Tensor ws = scratch(nb, log_w);
    chk(fn(fp(log_w, "log_w"), n, (uint64_t)seed, n_samples, (int32_t)order, idx.data_ptr<int64_t>(), aligned(ws), nb,
           stream_of(log_w)),
        name);
    return idx;
}

// Seeded stratified resampling indices (fabhip_resample_stratified): non-decreasing for order = 0.
Tensor resample_stratified(const Tensor& log_w, int64_t seed, int64_t n_samples, int64_t order) {
    return resample_seeded(fabhip_resample_stratified_workspace_bytes, fabhip_resample_stratified, "resample_stratified", log_w,
                           seed, n_samples, order);
}

// seeded streaming multinomial (fabhip_resample_multinomial_stream)
Tensor resample_multinomial_stream(const Tensor& log_w, int64_t seed, int64_t n_samples, int64_t order) {
    return resample_seeded(fabhip_resample_stream_workspace_bytes, fabhip_resample_multinomial_stream,
                           "resample_multinomial_stream", log_w, seed, n_samples, order);
}

Tensor multinomial_torch(const Tensor& probs, const Tensor& u) {
    c10::DeviceGuard g(probs.device());
    need(u, at::kDouble, "u");
    const int64_t n = probs.numel(), ns = u.numel();
    Tensor idx = at::empty({ns}, probs.options().dtype(at::kLong));
    const size_t nb = fabhip_multinomial_torch_workspace_bytes(n);
    Tensor ws = scratch(nb, probs);
    chk(fabhip_multinomial_torch(fp(probs, "probs"), n, u.data_ptr<double>(), ns, idx.data_ptr<int64_t>(), aligned(ws),
                                 nb, stream_of(probs)),
        "multinomial_torch");
    return idx;
}

Tensor gather_rows(const Tensor& src, const Tensor& idx) {
    c10::DeviceGuard g(src.device());
    need(idx, at::kLong, "idx");
    TORCH_CHECK(src.dim() >= 1, "fabhip: gather_rows needs at least one dimension");
    const int64_t rows = src.size(0), row_len = rows ? src.numel() / rows : 0, n_out = idx.numel();
    std::vector<int64_t> shape(src.sizes().begin(), src.sizes().end());
    shape[0] = n_out;
    Tensor out = at::empty(shape, src.options());
    if (n_out == 0 || row_len == 0) return out;
    chk(fabhip_gather_rows(fp(src, "src"), idx.data_ptr<int64_t>(), out.data_ptr<float>(), n_out, row_len,
                           stream_of(src)),
        "gather_rows");
    return out;
}

// PrioritisedReplayBuffer.add / the row selection of .sample as one op each (the draws come from torch's device generator)
void buffer_add(const Tensor& x, const Tensor& log_w, const Tensor& log_q_old, int64_t start, Tensor buf_x, Tensor buf_log_w,
                Tensor buf_log_q_old) {
    c10::DeviceGuard g(buf_x.device());
    TORCH_CHECK(x.dim() == 2 && buf_x.dim() == 2 && x.size(1) == buf_x.size(1), "fabhip: x must be [n, dim] like the buffer");
    const int64_t n = x.size(0), dim = x.size(1), L = buf_x.size(0);
    need_n(log_w, n, buf_x, "log_w"); need_n(log_q_old, n, buf_x, "log_q_old");
    need_n(buf_log_w, L, buf_x, "buffer log_w"); need_n(buf_log_q_old, L, buf_x, "buffer log_q_old");
    need_n(x, n * dim, buf_x, "x");
    chk(fabhip_buffer_add(fp(x, "x"), fp(log_w, "log_w"), fp(log_q_old, "log_q_old"), n, (int32_t)dim, start, L, fpm(buf_x, "buffer x"),
                          fpm(buf_log_w, "buffer log_w"), fpm(buf_log_q_old, "buffer log_q_old"), stream_of(buf_x)),
        "buffer_add");
}

Tensor buffer_sample_indices(const Tensor& log_w, int64_t k) {
    c10::DeviceGuard g(log_w.device());
    const int64_t n = log_w.numel();
    Tensor u = at::rand({n}, log_w.options().dtype(at::kFloat)), r = at::rand({4}, log_w.options().dtype(at::kFloat));
    Tensor idx = at::empty({k}, log_w.options().dtype(at::kLong));
    const size_t nb = fabhip_buffer_sample_workspace_bytes(n, k);
    TORCH_CHECK(nb > 0, "fabhip: buffer_sample_indices needs 1 <= k <= n");
    Tensor ws = scratch(nb, log_w);
    chk(fabhip_buffer_sample(fp(log_w, "log_w"), u.data_ptr<float>(), r.data_ptr<float>(), n, k, idx.data_ptr<int64_t>(), aligned(ws),
                             nb, stream_of(log_w)),
        "buffer_sample");
    return idx;
}

Tensor topk(const Tensor& keys, int64_t k, bool sorted) {
    c10::DeviceGuard g(keys.device());
    const int64_t n = keys.numel();
    Tensor idx = at::empty({k}, keys.options().dtype(at::kLong));
    const size_t nb = fabhip_topk_workspace_bytes(n, k);
    Tensor ws = scratch(nb, keys);
    chk(fabhip_topk(fp(keys, "keys"), n, k, sorted ? 1 : 0, idx.data_ptr<int64_t>(), nullptr, aligned(ws), nb,
                    stream_of(keys)),
        "topk");
    return idx;
}

}  // namespace

#define TGT "int target_kind, float[] target_params, Tensor? locs, Tensor? scales"
#define FLW "Tensor packed, int dim, int n_layers, int width"
// the parameters ais_run / ais_run_ext and ais_phase / ais_phase_smc share, up to and including `int precision`
#define AIS_RUN FLW ", " TGT ", float[] betas, float alpha, bool p_target, int transition, Tensor eps0, "                      \
    "Tensor? noise_a, Tensor? noise_b, Tensor(a!) step_state, Tensor(b!)? common_epsilon, Tensor? mass, int n_inner, "         \
    "int L, float max_grad, float target_p_accept, bool tune, Tensor(c!)? p_accept_first, Tensor(d!)? p_accept_last, "         \
    "Tensor(e!)? avg_distance_first, Tensor(f!)? avg_distance_last, bool want_base, int precision"
#define AIS_PHASE FLW ", " TGT ", float[] betas, float alpha, bool p_target, int transition, int phases, int j_begin, "        \
    "int j_end, Tensor? eps0, Tensor noise_a, Tensor noise_b, Tensor(a!) step_state, Tensor(b!)? common_epsilon, "             \
    "Tensor? mass, int n_inner, int L, float max_grad, float target_p_accept, bool tune, Tensor(c!) x, "                       \
    "Tensor(d!) log_q, Tensor(e!) log_p, Tensor(f!)? grad_log_q, Tensor(g!)? grad_log_p, Tensor(h!) log_w, "                   \
    "Tensor(i!) n_valid, Tensor(j!) stats, Tensor(k!)? partials, Tensor(l!)? p_accept_first, "                                 \
    "Tensor(m!)? p_accept_last, Tensor(n!)? avg_distance_first, Tensor(o!)? avg_distance_last, Tensor(p!)? base_x, "           \
    "Tensor(q!)? base_log_w, int precision"

TORCH_LIBRARY(fabhip, m) {
    m.def("abi_version() -> int", abi_version);
    m.def("flow_packed_floats(int dim, int n_layers, int width) -> int", flow_packed_floats);
    m.def("tensors_key(Tensor[] ts) -> int[]", tensors_key);
    m.def("tensors_key_register(Tensor[] ts, int reuse) -> int", tensors_key_register);
    m.def("tensors_key_of(int handle) -> int[]", tensors_key_of);
    m.def("tensors_key_release(int handle) -> ()", tensors_key_release);
    m.def("flow_grad_floats(int dim, int n_layers, int width) -> int", flow_grad_floats);
    m.def("flow_grad_layout(int dim, int n_layers, int width) -> int[]", flow_grad_layout);
    m.def("flow_tape_layout(int dim, int n_layers, int width, int B) -> int[]", flow_tape_layout);
    m.def("train_step_plan(int dim, int n_layers, int width) -> int[]", train_step_plan);
    m.def("set_fast_mode(bool on) -> int", set_fast_mode);
    m.def("get_fast_mode() -> int", get_fast_mode);
    m.def("set_option(int key, int value) -> int", set_option);
    m.def("get_option(int key) -> int", get_option);
    m.def("anneal_coefs(float beta, float alpha, bool p_target) -> float[]", anneal_coefs);

    m.def("realnvp_pack(Tensor[] params, int dim, int n_layers, int width, bool with_inverse, Tensor(a!) packed) -> ()");
    m.def("realnvp_sample(" FLW ", Tensor eps) -> (Tensor, Tensor)");
    m.def("realnvp_logprob_grad(" FLW ", Tensor x, bool with_grad, int precision=0) -> (Tensor, Tensor)");
    m.def("realnvp_logprob_tape(Tensor theta, Tensor x, Tensor packed, Tensor[] params, int dim, int n_layers, "
          "int width, bool want_grad_x) -> (Tensor, Tensor, Tensor)");
    m.def("realnvp_param_grad(Tensor[] params, " FLW ", Tensor tape, Tensor coef) -> Tensor");
    m.def("realnvp_sample_tape(Tensor theta, Tensor eps, Tensor packed, Tensor[] params, int dim, int n_layers, "
          "int width) -> (Tensor, Tensor)");
    m.def("realnvp_sample_grad_tape(" FLW ", Tensor x, Tensor grad_x, Tensor grad_log_q) -> (Tensor, Tensor)");
    m.def("buffer_train_step(int pset, Tensor(a!) packed, int dim, int n_layers, int width, bool repack, Tensor x, Tensor? rows, "
          "Tensor log_q_old, bool log_q_old_rows, float alpha, float w_clip, Tensor(b!)? buf_log_w, Tensor(c!)? buf_log_q_old, "
          "Tensor(d!) theta, Tensor(e!) m, Tensor(f!) v, float lr, float beta1, float beta2, float eps, Tensor(g!) step_count, "
          "float max_norm) -> (Tensor, Tensor, Tensor)");
    m.def("adam_clip_step(Tensor(a!) theta, Tensor grad, Tensor(b!) m, Tensor(c!) v, float lr, float beta1, float beta2, "
          "float eps, Tensor(d!) step_count, float max_norm, Tensor(e!) grad_norm) -> ()");

    m.def("spline_packed_floats(int dim, int n_layers, int hidden) -> int", spline_packed_floats);
    m.def("spline_pack(Tensor[] params, int dim, int n_layers, int hidden, Tensor(a!) packed) -> ()");
    m.def("spline_logprob_grad(Tensor packed, int dim, int n_layers, int hidden, Tensor x, bool with_grad, int precision=0) -> (Tensor, Tensor)");
    m.def("spline_tape_layout(int dim, int n_layers, int hidden, int B) -> int[]", spline_tape_layout);
    m.def("spline_logprob_tape(Tensor packed, int dim, int n_layers, int hidden, Tensor x) -> (Tensor, Tensor, Tensor)");
    m.def("spline_sample(Tensor packed, int dim, int n_layers, int hidden, Tensor u, Tensor eps) -> (Tensor, Tensor)");
    m.def("spline_sample_vjp_tape(Tensor packed, int dim, int n_layers, int hidden, Tensor u, Tensor eps, Tensor? gx, Tensor? gl) -> (Tensor, Tensor, Tensor)");
    m.def("target_logp_grad(" TGT ", Tensor x, bool with_grad) -> (Tensor, Tensor)");
    m.def("manywell_logp_grad(Tensor x, float a, float b, float c, float log_norm) -> (Tensor, Tensor)");
    m.def("gmm_logp_grad(Tensor x, Tensor locs, Tensor scales) -> (Tensor, Tensor)");
    m.def("create_point(" FLW ", " TGT ", Tensor x, bool with_grad, int precision=0) -> (Tensor, Tensor, Tensor, Tensor)");

    m.def("hmc_transition(" FLW ", " TGT ", Tensor(a!) x, Tensor(b!) log_q, Tensor(c!) log_p, Tensor(d!) grad_log_q, "
          "Tensor(e!) grad_log_p, Tensor(f!)? log_w, float beta, float beta_next, float alpha, bool p_target, "
          "Tensor noise_p, Tensor noise_e, Tensor(g!) epsilons_row, Tensor(h!) common_epsilon, Tensor mass, int L, "
          "float max_grad, float target_p_accept, bool tune, Tensor(i!)? p_accept, Tensor(j!)? avg_distance, int precision=0) -> ()");
    m.def("metropolis_transition(" FLW ", " TGT ", Tensor(a!) x, Tensor(b!) log_q, Tensor(c!) log_p, Tensor(d!)? log_w, "
          "float beta, float beta_next, float alpha, bool p_target, Tensor noise_x, Tensor noise_u, "
          "Tensor(e!) noise_scalings_row, float target_p_accept, bool tune) -> ()");
    m.def("ais_run(" AIS_RUN "=0) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("ais_phase(" AIS_PHASE "=0) -> ()");
    m.def("ais_run_ext(" AIS_RUN ", float? tau=None, Tensor? noise_r=None, bool want_trace=False, int method=0, "
          "Tensor? mix_loc=None, Tensor? mix_log_scale=None, Tensor? mix_logit=None, Tensor? sel=None, bool mix_enabled=False, "
          "int n_moves=0, Tensor? noise_g=None, Tensor? noise_h=None) -> Tensor[]");
    m.def("flow_move(" FLW ", " TGT ", Tensor(a!) x, Tensor(b!) log_q, Tensor(c!) log_p, Tensor(d!)? grad_log_q, "
          "Tensor(e!)? grad_log_p, Tensor? n_valid, float beta, float alpha, bool p_target, Tensor noise_g, Tensor noise_h, "
          "int precision=0) -> (Tensor, Tensor)");
    m.def("defensive_log_prob(" FLW ", Tensor loc, Tensor log_scale, Tensor mixture_logit, Tensor x, bool with_grad, "
          "int precision=0) -> (Tensor, Tensor)");
    m.def("ais_phase_smc(" AIS_PHASE ", float? tau, Tensor? noise_r, bool only_resample, Tensor(r!)? resampled, "
          "Tensor(s!)? ess, Tensor(t!)? ancestors, Tensor(u!)? log_w_pre, int method=0) -> ()");
    m.def("smc_decide(Tensor log_w, float tau, Tensor u, int method=0) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("next_beta(Tensor log_w, Tensor log_q, Tensor log_p, Tensor? n_valid, float beta, float alpha, bool p_target, "
          "float rho, int iters=24) -> Tensor");
    m.def("log_w_first(Tensor log_q, Tensor log_p, float beta_next, float alpha, bool p_target, Tensor(a!) log_w) -> ()");
    m.def("smc_shard_pack(Tensor x, Tensor log_q, Tensor log_p, Tensor? grad_log_q, Tensor? grad_log_p, Tensor log_w, "
          "Tensor n_valid) -> Tensor");
    m.def("smc_shard_resample(Tensor gathered, int world, int rank, float tau, Tensor u, Tensor(a!) x, Tensor(b!) log_q, "
          "Tensor(c!) log_p, Tensor(d!)? grad_log_q, Tensor(e!)? grad_log_p, Tensor(f!) log_w, Tensor n_valid, "
          "bool want_trace) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("ais_sharded_tuned(" FLW ", " TGT ", float[] betas, float alpha, bool p_target, int transition, Tensor? eps0, "
          "Tensor noise_a, Tensor noise_b, Tensor(a!) step_state, Tensor(b!)? common_epsilon, Tensor? mass, int L, "
          "float max_grad, float target_p_accept, Tensor(c!) x, Tensor(d!) log_q, Tensor(e!) log_p, Tensor(f!)? grad_log_q, "
          "Tensor(g!)? grad_log_p, Tensor(h!) log_w, Tensor(i!) n_valid, Tensor(j!) stats, Tensor(k!) partials, "
          "Tensor(l!)? p_accept_first, Tensor(m!)? p_accept_last, Tensor(n!)? avg_distance_first, "
          "Tensor(o!)? avg_distance_last, int precision, str group_name) -> int");
    m.def("hmc_partials_floats(int B) -> int", hmc_partials_floats);
    m.def("metropolis_partials_floats(int B, int M, int n_updates) -> int", metropolis_partials_floats);
    m.def("metropolis_adapt_gathered(Tensor gathered, int n_ranks, int B_rank, Tensor(a!) noise_scalings, "
          "float target_p_accept, bool tune) -> ()");
    m.def("tape_gemm(Tensor tape, int layer_stride, int L, int off_y, int ldy, int P, int off_x, int ldx, int Q, Tensor coef, "
          "bool want_colsum) -> (Tensor, Tensor)");
    m.def("hmc_adapt_gathered(Tensor gathered, int n_ranks, int B_rank, Tensor(a!) epsilon, Tensor(b!) common_epsilon, "
          "float target_p_accept, bool tune, Tensor(c!)? p_accept, Tensor(d!)? avg_distance) -> ()");
    m.def("generic_workspace(Tensor like, int B, int dim) -> Tensor");
    m.def("hmc_generic_begin(Tensor start_x, Tensor start_gq, Tensor start_gp, Tensor cur_lq, Tensor cur_lp, float beta, "
          "float alpha, bool p_target, Tensor noise_p, Tensor mass, float max_grad, Tensor(a!) ws) -> ()");
    m.def("hmc_generic_leap_pre(int B, int dim, Tensor eps, Tensor ceps, Tensor mass, Tensor(a!) ws) -> Tensor");
    m.def("hmc_generic_leap_post(Tensor gq, Tensor gp, float beta, float alpha, bool p_target, float max_grad, Tensor eps, "
          "Tensor ceps, Tensor(a!) ws) -> ()");
    m.def("hmc_generic_accept(Tensor prop_lq, Tensor prop_lp, Tensor prop_gq, Tensor prop_gp, Tensor(a!) x, "
          "Tensor(b!) log_q, Tensor(c!) log_p, Tensor(d!) grad_log_q, Tensor(e!) grad_log_p, Tensor(f!)? log_w, float beta, "
          "float beta_next, float alpha, bool p_target, Tensor noise_e, Tensor mass, Tensor(g!) eps, Tensor(h!) ceps, "
          "float target_p_accept, bool tune, Tensor(i!)? p_accept, Tensor(j!)? avg_distance, Tensor(k!) ws) -> ()");
    m.def("spline_hmc_transition(Tensor packed, int dim, int n_layers, int hidden, int target_kind, float[] target_params, "
          "Tensor? locs, Tensor? scales, Tensor(a!) x, Tensor(b!) log_q, Tensor(c!) log_p, Tensor(d!) grad_log_q, "
          "Tensor(e!) grad_log_p, Tensor(f!)? log_w, float beta, float beta_next, float alpha, bool p_target, Tensor noise_p, "
          "Tensor noise_e, Tensor(g!) eps_row, Tensor(h!) ceps, Tensor mass, int n_outer, int n_leap, float max_grad, "
          "float target_p_accept, bool tune, Tensor(i!)? p_accept, Tensor(j!)? avg_distance, int precision=0) -> ()");
    m.def("spline_ais_run(Tensor packed, int dim, int n_layers, int hidden, " TGT ", float[] betas, float alpha, bool p_target, "
          "Tensor u0, Tensor eps0, Tensor noise_p, Tensor noise_e, Tensor(a!) epsilons, Tensor(b!) common_epsilon, Tensor mass, "
          "int n_outer, int L, float max_grad, float target_p_accept, bool tune, Tensor(c!)? p_accept_first, "
          "Tensor(d!)? p_accept_last, Tensor(e!)? avg_distance_first, Tensor(f!)? avg_distance_last, bool want_base, int precision=0) -> "
          "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("anneal_log_prob(Tensor log_q, Tensor log_p, float beta, float alpha, bool p_target) -> Tensor");
    m.def("log_w_update(Tensor log_q, Tensor log_p, float beta, float beta_next, float alpha, bool p_target, "
          "Tensor(a!) log_w) -> ()");
    m.def("metropolis_generic_propose(Tensor x, Tensor noise_x, Tensor scale) -> Tensor");
    m.def("metropolis_generic_accept(Tensor x_new, Tensor new_lq, Tensor new_lp, Tensor(a!) x, Tensor(b!) log_q, "
          "Tensor(c!) log_p, Tensor prev_log_prob, Tensor noise_u, float beta, float alpha, bool p_target, "
          "Tensor(d!) scale, float target_p_accept, bool tune) -> ()");

    m.def("ess_logz(Tensor log_w, Tensor? n_ptr, float n_norm) -> Tensor");
    m.def("fixed_cdf(Tensor log_w, Tensor(a!)? workspace) -> Tensor(a!)");
    m.def("resample_multinomial(Tensor log_w, Tensor u) -> Tensor");
    m.def("resample_systematic(Tensor log_w, float u0, int n_samples) -> Tensor");
    m.def("resample_multinomial_stream(Tensor log_w, int seed, int n_samples, int order) -> Tensor");
    m.def("resample_stratified(Tensor log_w, int seed, int n_samples, int order) -> Tensor");
    m.def("multinomial_torch(Tensor probs, Tensor u) -> Tensor");
    m.def("gather_rows(Tensor src, Tensor idx) -> Tensor");
    m.def("topk(Tensor keys, int k, bool sorted) -> Tensor");
    m.def("buffer_add(Tensor x, Tensor log_w, Tensor log_q_old, int start, Tensor(a!) buf_x, Tensor(b!) buf_log_w, "
          "Tensor(c!) buf_log_q_old) -> ()");
    m.def("buffer_sample_indices(Tensor log_w, int k) -> Tensor");
}

TORCH_LIBRARY_IMPL(fabhip, CUDA, m) {      // CUDA == HIP on PyTorch-ROCm; deliberately no CPU registration
    m.impl("realnvp_pack", realnvp_pack);
    m.impl("realnvp_sample", realnvp_sample);
    m.impl("realnvp_logprob_grad", realnvp_logprob_grad);
    m.impl("realnvp_logprob_tape", realnvp_logprob_tape);
    m.impl("realnvp_param_grad", realnvp_param_grad);
    m.impl("realnvp_sample_tape", realnvp_sample_tape);
    m.impl("realnvp_sample_grad_tape", realnvp_sample_grad_tape);
    m.impl("adam_clip_step", adam_clip_step);
    m.impl("buffer_train_step", buffer_train_step);
    m.impl("spline_pack", spline_pack);
    m.impl("spline_logprob_grad", spline_logprob_grad);
    m.impl("spline_logprob_tape", spline_logprob_tape);
    m.impl("spline_sample", spline_sample);
    m.impl("spline_sample_vjp_tape", spline_sample_vjp_tape);
    m.impl("target_logp_grad", target_logp_grad);
    m.impl("manywell_logp_grad", manywell_logp_grad);
    m.impl("gmm_logp_grad", gmm_logp_grad);
    m.impl("create_point", create_point);
    m.impl("hmc_transition", hmc_transition);
    m.impl("metropolis_transition", metropolis_transition);
    m.impl("ais_run", ais_run);
    m.impl("ais_phase", ais_phase);
    m.impl("ais_run_ext", ais_run_ext);
    m.impl("ais_phase_smc", ais_phase_smc);
    m.impl("flow_move", flow_move);
    m.impl("defensive_log_prob", defensive_log_prob);
    m.impl("smc_decide", smc_decide);
    m.impl("next_beta", next_beta);
    m.impl("log_w_first", log_w_first);
    m.impl("smc_shard_pack", smc_shard_pack);
    m.impl("smc_shard_resample", smc_shard_resample);
    m.impl("ais_sharded_tuned", ais_sharded_tuned);
    m.impl("metropolis_adapt_gathered", metropolis_adapt_gathered);
    m.impl("tape_gemm", tape_gemm);
    m.impl("spline_ais_run", spline_ais_run);
    m.impl("hmc_adapt_gathered", hmc_adapt_gathered);
    m.impl("generic_workspace", generic_workspace);
    m.impl("hmc_generic_begin", hmc_generic_begin);
    m.impl("hmc_generic_leap_pre", hmc_generic_leap_pre);
    m.impl("hmc_generic_leap_post", hmc_generic_leap_post);
    m.impl("hmc_generic_accept", hmc_generic_accept);
    m.impl("spline_hmc_transition", spline_hmc_transition);
    m.impl("anneal_log_prob", anneal_log_prob);
    m.impl("log_w_update", log_w_update);
    m.impl("metropolis_generic_propose", metropolis_generic_propose);
    m.impl("metropolis_generic_accept", metropolis_generic_accept);
    m.impl("ess_logz", ess_logz);
    m.impl("fixed_cdf", fixed_cdf);
    m.impl("resample_multinomial", resample_multinomial);
    m.impl("resample_systematic", resample_systematic);
    m.impl("resample_multinomial_stream", resample_multinomial_stream);
    m.impl("resample_stratified", resample_stratified);
    m.impl("multinomial_torch", multinomial_torch);
    m.impl("gather_rows", gather_rows);
    m.impl("topk", topk);
    m.impl("buffer_add", buffer_add);
    m.impl("buffer_sample_indices", buffer_sample_indices);
}
