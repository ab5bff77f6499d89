// optim.hip -- the optimiser step of the training recipe (nn/meta/arch.py:48-75: torch.optim.AdamW; gradient clipping at
// 35.0 = conf/trainer/train.yaml gradient_clip_val) for ALL parameters in two launches: (1) per-chunk sums of squares of the
// gradients, (2) total norm -> clip coefficient -> decoupled weight decay + Adam update of every chunk.  Replaces ATen's
// clip_grad_norm_ (foreach norm, stack, norm, clamp, foreach mul) + foreach AdamW (~10 multi-tensor launches that move
// each of p, g, m, v several times).  HBM-bound: g is read twice, p / m / v once and written once, 16-byte accesses.
//
// The arithmetic follows torch/optim/adamw.py (_multi_tensor_adamw, non-capturable) operation by operation in fp32:
//   p *= 1 - lr*wd;  m = m + (g - m)(1 - b1);  v = v*b2 + g*g*(1 - b2);
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// with g = grad * min(1, max_norm / (||grad||_2 + 1e-6)) (torch.nn.utils.clip_grad_norm_).
//
// rv_adamw_step_groups (include/rv3d_optim.h) is the same pair of launches for several parameter groups, per-parameter step
// counts, amsgrad and maximize: the hyper-parameters become rows passed by value, each tensor names its row.
#include "common.h"
#include "../../include/rv3d_optim.h"

namespace {

constexpr int kChunk = 65536;  // elements per workgroup

struct OptTensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
};
struct OptChunk {
    int32_t tensor, chunk;
};

__global__ __launch_bounds__(256) void optim_sqnorm_kernel(const OptTensor* tensors, const OptChunk* chunks, float* partial) {
    const OptChunk c = chunks[blockIdx.x];
    const OptTensor t = tensors[c.tensor];
    const int64_t lo = (int64_t)c.chunk * kChunk, hi = lo + kChunk < t.n ? lo + kChunk : t.n;
    const float* g = t.g + lo;
    const int64_t n = hi - lo;
    float s = 0.f;
    if ((((uintptr_t)g) & 15) == 0) {
        const int64_t n4 = n >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += 256) {
            const f32x4 x = ((const f32x4*)g)[i];
            s += x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
        }
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) s += g[i] * g[i];
    } else {
        for (int64_t i = threadIdx.x; i < n; i += 256) s += g[i] * g[i];
    }
    __shared__ float red[4];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct OptHyper {  // the scalars torch forms in double on the host, each rounded to fp32 once (as the foreach ops take them)
    float decay, one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps, max_norm;
};

__device__ __forceinline__ void adam_elem(float& p, const float g, float& m, float& v, const OptHyper& h, const float clip) {
    const float gc = g * clip;
    p *= h.decay;
    m = m + (gc - m) * h.one_minus_beta1;
    v = v * h.beta2 + gc * gc * h.one_minus_beta2;
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    p -= h.step_size * (m / denom);
}

__global__ __launch_bounds__(256) void optim_adamw_kernel(const OptTensor* tensors, const OptChunk* chunks, const float* partial,
                                                          int n_partial, const OptHyper h, float* total_norm_out) {
    // every workgroup forms the same total (fixed order: reproducible) from the per-chunk sums
    __shared__ double red[4];
    __shared__ float clip_s;
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += 256) s += (double)partial[i];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
        float clip = 1.f;
        if (h.max_norm > 0.f) {
            clip = h.max_norm / (norm + 1e-6f);
            clip = clip < 1.f ? clip : 1.f;
        }
        clip_s = clip;
        if (blockIdx.x == 0 && total_norm_out) total_norm_out[0] = norm;
    }
    __syncthreads();
    const float clip = clip_s;
    const OptChunk c = chunks[blockIdx.x];
    const OptTensor t = tensors[c.tensor];
    const int64_t lo = (int64_t)c.chunk * kChunk, hi = lo + kChunk < t.n ? lo + kChunk : t.n;
    const int64_t n = hi - lo;
    float* p = t.p + lo;
    const float* g = t.g + lo;
    float* m = t.m + lo;
    float* v = t.v + lo;
    int64_t done = 0;
    if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0) {
        const int64_t n4 = n >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += 256) {
            const f32x4 p4 = ((f32x4*)p)[i], m4 = ((f32x4*)m)[i], v4 = ((f32x4*)v)[i], g4 = ((const f32x4*)g)[i];
            float pp[4] = {p4[0], p4[1], p4[2], p4[3]}, mm[4] = {m4[0], m4[1], m4[2], m4[3]}, vv[4] = {v4[0], v4[1], v4[2], v4[3]};
            const float gg[4] = {g4[0], g4[1], g4[2], g4[3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) adam_elem(pp[j], gg[j], mm[j], vv[j], h, clip);
            ((f32x4*)p)[i] = f32x4{pp[0], pp[1], pp[2], pp[3]};
            ((f32x4*)m)[i] = f32x4{mm[0], mm[1], mm[2], mm[3]};
            ((f32x4*)v)[i] = f32x4{vv[0], vv[1], vv[2], vv[3]};
        }
        done = n4 << 2;
    }
    for (int64_t i = done + threadIdx.x; i < n; i += 256) adam_elem(p[i], g[i], m[i], v[i], h, clip);
}

// ---- the same step for several parameter groups / step counts / amsgrad / maximize (rv_adamw_step_groups, rv3d_optim.h) ----
constexpr int kMaxRows = 64;  // rows of hyper-parameters by value in the kernel arguments: 64 x 32 B = 2 KB of the 4 KB there are

struct OptRow {  // OptHyper of one (group, step count), without max_norm (one for all rows) and with the row's RV_ADAM_* flags
    float decay, one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps;
    int32_t flags;
};
struct OptRows {
    OptRow r[kMaxRows];
};

// adam_elem with amsgrad: vmax = max(vmax, v) (_foreach_maximum_), and the denominator takes sqrt(vmax)
__device__ __forceinline__ void adam_elem_amsgrad(float& p, const float g, float& m, float& v, float& vmax, const OptHyper& h, const float clip) {
    const float gc = g * clip;
    p *= h.decay;
    m = m + (gc - m) * h.one_minus_beta1;
    v = v * h.beta2 + gc * gc * h.one_minus_beta2;
    vmax = (vmax != vmax || vmax > v) ? vmax : v;  // at::maximum: a NaN on either side is kept
    const float denom = sqrtf(vmax) / h.bc2_sqrt + h.eps;
    p -= h.step_size * (m / denom);
}

__global__ __launch_bounds__(256) void optim_adamw_groups_kernel(const OptTensor* tensors, const int32_t* tensor_row, float* const* vmax,
                                                                 const OptChunk* chunks, const float* partial, int n_partial,
                                                                 const float max_norm, const int n_rows, float* total_norm_out,
                                                                 const OptRows rows) {
    // the total and the clip coefficient as optim_adamw_kernel forms them (same order, same operations)
    __shared__ double red[4];
    __shared__ float clip_s;
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += 256) s += (double)partial[i];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
        float clip = 1.f;
        if (max_norm > 0.f) {
            clip = max_norm / (norm + 1e-6f);
            clip = clip < 1.f ? clip : 1.f;
        }
        clip_s = clip;
        if (blockIdx.x == 0 && total_norm_out) total_norm_out[0] = norm;
    }
    __syncthreads();
    const OptChunk c = chunks[blockIdx.x];
    const OptTensor t = tensors[c.tensor];
    const int32_t ri = tensor_row[c.tensor];
    if (ri < 0 || ri >= n_rows) return;  // (uniform; the host checks the column: never index the by-value array outside it)
    const OptRow r = rows.r[ri];
    OptHyper h;
    h.decay = r.decay;
    h.one_minus_beta1 = r.one_minus_beta1;
    h.beta2 = r.beta2;
    h.one_minus_beta2 = r.one_minus_beta2;
    h.step_size = r.step_size;
    h.bc2_sqrt = r.bc2_sqrt;
    h.eps = r.eps;
    h.max_norm = max_norm;
    // maximize: g = -g before anything else; (-g) * clip == g * (-clip) exactly, so the sign rides on the coefficient
    const float clip = (r.flags & RV_ADAM_MAXIMIZE) ? -clip_s : clip_s;
    const int64_t lo = (int64_t)c.chunk * kChunk, hi = lo + kChunk < t.n ? lo + kChunk : t.n;
    const int64_t n = hi - lo;
    float* p = t.p + lo;
    const float* g = t.g + lo;
    float* m = t.m + lo;
    float* v = t.v + lo;
    int64_t done = 0;
    if (r.flags & RV_ADAM_AMSGRAD) {
        float* x = vmax ? vmax[c.tensor] : nullptr;
        if (x == nullptr) return;  // (uniform; the entry point refuses amsgrad rows without the table)
        x += lo;
        if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)x)) & 15) == 0) {
            const int64_t n4 = n >> 2;
            for (int64_t i = threadIdx.x; i < n4; i += 256) {
                const f32x4 p4 = ((f32x4*)p)[i], m4 = ((f32x4*)m)[i], v4 = ((f32x4*)v)[i], x4 = ((f32x4*)x)[i], g4 = ((const f32x4*)g)[i];
                float pp[4] = {p4[0], p4[1], p4[2], p4[3]}, mm[4] = {m4[0], m4[1], m4[2], m4[3]}, vv[4] = {v4[0], v4[1], v4[2], v4[3]};
                float xx[4] = {x4[0], x4[1], x4[2], x4[3]};
                const float gg[4] = {g4[0], g4[1], g4[2], g4[3]};
#pragma unroll
                for (int j = 0; j < 4; ++j) adam_elem_amsgrad(pp[j], gg[j], mm[j], vv[j], xx[j], h, clip);
                ((f32x4*)p)[i] = f32x4{pp[0], pp[1], pp[2], pp[3]};
                ((f32x4*)m)[i] = f32x4{mm[0], mm[1], mm[2], mm[3]};
                ((f32x4*)v)[i] = f32x4{vv[0], vv[1], vv[2], vv[3]};
                ((f32x4*)x)[i] = f32x4{xx[0], xx[1], xx[2], xx[3]};
            }
            done = n4 << 2;
        }
        for (int64_t i = done + threadIdx.x; i < n; i += 256) adam_elem_amsgrad(p[i], g[i], m[i], v[i], x[i], h, clip);
        return;
    }
    if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0) {
        const int64_t n4 = n >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += 256) {
            const f32x4 p4 = ((f32x4*)p)[i], m4 = ((f32x4*)m)[i], v4 = ((f32x4*)v)[i], g4 = ((const f32x4*)g)[i];
            float pp[4] = {p4[0], p4[1], p4[2], p4[3]}, mm[4] = {m4[0], m4[1], m4[2], m4[3]}, vv[4] = {v4[0], v4[1], v4[2], v4[3]};
            const float gg[4] = {g4[0], g4[1], g4[2], g4[3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) adam_elem(pp[j], gg[j], mm[j], vv[j], h, clip);
            ((f32x4*)p)[i] = f32x4{pp[0], pp[1], pp[2], pp[3]};
            ((f32x4*)m)[i] = f32x4{mm[0], mm[1], mm[2], mm[3]};
            ((f32x4*)v)[i] = f32x4{vv[0], vv[1], vv[2], vv[3]};
        }
        done = n4 << 2;
    }
    for (int64_t i = done + threadIdx.x; i < n; i += 256) adam_elem(p[i], g[i], m[i], v[i], h, clip);
}

// ---- weight averaging (EMA / SWA: torch.optim.swa_utils.AveragedModel) in the step's second launch (rv_adamw_step_groups_avg) and as a
// launch of its own for the tensors the optimiser did not step (rv_average_tensors); rv3d_optim.h ----
// at::lerp's expression (ATen/native/Lerp.h) in fp32; w == 1 gives p - (p - a) * 0 = p exactly
__device__ __forceinline__ float avg_lerp(const float a, const float p, const float w) {
    return w < 0.5f ? a + w * (p - a) : p - (p - a) * (1.f - w);
}

// One chunk of the step.  AMS: the row carries RV_ADAM_AMSGRAD (x = max_exp_avg_sq); AVG: the tensor has an averaged twin `a`, updated
// from the new p while it is in registers.  The element functions are those of optim_adamw_groups_kernel, so p / m / v / x come out
// bit for bit as there.  The 16-byte path needs every pointer of the chunk aligned, `a` included.
template <bool AMS, bool AVG>
__device__ __forceinline__ void adam_chunk_avg(float* p, const float* g, float* m, float* v, float* x, float* a, const int64_t n,
                                               const OptHyper& h, const float clip, const float w) {
    uintptr_t bits = ((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v);
    if (AMS) bits |= (uintptr_t)x;
    if (AVG) bits |= (uintptr_t)a;
    int64_t done = 0;
    if ((bits & 15) == 0) {
        const int64_t n4 = n >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += 256) {
            const f32x4 p4 = ((f32x4*)p)[i], m4 = ((f32x4*)m)[i], v4 = ((f32x4*)v)[i], g4 = ((const f32x4*)g)[i];
            f32x4 x4 = {0.f, 0.f, 0.f, 0.f}, a4 = {0.f, 0.f, 0.f, 0.f};
            if (AMS) x4 = ((f32x4*)x)[i];
            if (AVG) a4 = ((f32x4*)a)[i];
            float pp[4] = {p4[0], p4[1], p4[2], p4[3]}, mm[4] = {m4[0], m4[1], m4[2], m4[3]}, vv[4] = {v4[0], v4[1], v4[2], v4[3]};
            float xx[4] = {x4[0], x4[1], x4[2], x4[3]}, aa[4] = {a4[0], a4[1], a4[2], a4[3]};
            const float gg[4] = {g4[0], g4[1], g4[2], g4[3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (AMS) adam_elem_amsgrad(pp[j], gg[j], mm[j], vv[j], xx[j], h, clip);
                else adam_elem(pp[j], gg[j], mm[j], vv[j], h, clip);
                if (AVG) aa[j] = avg_lerp(aa[j], pp[j], w);
            }
            ((f32x4*)p)[i] = f32x4{pp[0], pp[1], pp[2], pp[3]};
            ((f32x4*)m)[i] = f32x4{mm[0], mm[1], mm[2], mm[3]};
            ((f32x4*)v)[i] = f32x4{vv[0], vv[1], vv[2], vv[3]};
            if (AMS) ((f32x4*)x)[i] = f32x4{xx[0], xx[1], xx[2], xx[3]};
            if (AVG) ((f32x4*)a)[i] = f32x4{aa[0], aa[1], aa[2], aa[3]};
        }
        done = n4 << 2;
    }
    for (int64_t i = done + threadIdx.x; i < n; i += 256) {
        if (AMS) adam_elem_amsgrad(p[i], g[i], m[i], v[i], x[i], h, clip);
        else adam_elem(p[i], g[i], m[i], v[i], h, clip);
        if (AVG) a[i] = avg_lerp(a[i], p[i], w);
    }
}

__global__ __launch_bounds__(256) void optim_adamw_groups_avg_kernel(const OptTensor* tensors, const int32_t* tensor_row, float* const* vmax,
                                                                     float* const* avg, const float avg_w, const OptChunk* chunks,
                                                                     const float* partial, int n_partial, const float max_norm,
                                                                     const int n_rows, float* total_norm_out, const OptRows rows) {
    // the total and the clip coefficient as optim_adamw_kernel forms them (same order, same operations)
    __shared__ double red[4];
    __shared__ float clip_s;
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += 256) s += (double)partial[i];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
        float clip = 1.f;
        if (max_norm > 0.f) {
            clip = max_norm / (norm + 1e-6f);
            clip = clip < 1.f ? clip : 1.f;
        }
        clip_s = clip;
        if (blockIdx.x == 0 && total_norm_out) total_norm_out[0] = norm;
    }
    __syncthreads();
    const OptChunk c = chunks[blockIdx.x];
    const OptTensor t = tensors[c.tensor];
    const int32_t ri = tensor_row[c.tensor];
    if (ri < 0 || ri >= n_rows) return;  // (uniform; as optim_adamw_groups_kernel)
    const OptRow r = rows.r[ri];
    OptHyper h;
    h.decay = r.decay;
    h.one_minus_beta1 = r.one_minus_beta1;
    h.beta2 = r.beta2;
    h.one_minus_beta2 = r.one_minus_beta2;
    h.step_size = r.step_size;
    h.bc2_sqrt = r.bc2_sqrt;
    h.eps = r.eps;
    h.max_norm = max_norm;
    const float clip = (r.flags & RV_ADAM_MAXIMIZE) ? -clip_s : clip_s;
    const int64_t lo = (int64_t)c.chunk * kChunk, hi = lo + kChunk < t.n ? lo + kChunk : t.n;
    const int64_t n = hi - lo;
    float* a = avg[c.tensor];  // NULL: this tensor is not averaged
    if (a) a += lo;
    float* x = nullptr;
    if (r.flags & RV_ADAM_AMSGRAD) {
        x = vmax ? vmax[c.tensor] : nullptr;
        if (x == nullptr) return;  // (uniform; the entry point refuses amsgrad rows without the table)
        x += lo;
    }
    // (all four choices are uniform over the workgroup)
    if (x) {
        if (a) adam_chunk_avg<true, true>(t.p + lo, t.g + lo, t.m + lo, t.v + lo, x, a, n, h, clip, avg_w);
        else adam_chunk_avg<true, false>(t.p + lo, t.g + lo, t.m + lo, t.v + lo, x, a, n, h, clip, avg_w);
    } else {
        if (a) adam_chunk_avg<false, true>(t.p + lo, t.g + lo, t.m + lo, t.v + lo, x, a, n, h, clip, avg_w);
        else adam_chunk_avg<false, false>(t.p + lo, t.g + lo, t.m + lo, t.v + lo, x, a, n, h, clip, avg_w);
    }
}

struct AvgTensor {  // one row of rv_average_tensors' table
    float* a;
    const float* src;
    int64_t n;
};

__global__ __launch_bounds__(256) void average_tensors_kernel(const AvgTensor* tensors, const OptChunk* chunks, const float w) {
    const OptChunk c = chunks[blockIdx.x];
    const AvgTensor t = tensors[c.tensor];
    const int64_t lo = (int64_t)c.chunk * kChunk;
    if (t.a == nullptr || t.src == nullptr || c.chunk < 0 || lo >= t.n) return;  // (uniform; a bad row is left untouched)
    const int64_t hi = lo + kChunk < t.n ? lo + kChunk : t.n;
    const int64_t n = hi - lo;
    float* a = t.a + lo;
    const float* p = t.src + lo;
    int64_t done = 0;
    if (((((uintptr_t)a) | ((uintptr_t)p)) & 15) == 0) {
        const int64_t n4 = n >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += 256) {
            const f32x4 a4 = ((f32x4*)a)[i], p4 = ((const f32x4*)p)[i];
            ((f32x4*)a)[i] = f32x4{avg_lerp(a4[0], p4[0], w), avg_lerp(a4[1], p4[1], w), avg_lerp(a4[2], p4[2], w), avg_lerp(a4[3], p4[3], w)};
        }
        done = n4 << 2;
    }
    for (int64_t i = done + threadIdx.x; i < n; i += 256) a[i] = avg_lerp(a[i], p[i], w);
}

}  // namespace

extern "C" int32_t rv_optim_chunk_elems(void) { return kChunk; }

extern "C" int rv_adamw_step(const void* tensors, const void* chunks, int32_t n_chunks, float* partial, double lr, double beta1,
                             double beta2, double eps, double weight_decay, int64_t step, double max_norm, float* total_norm,
                             rvStream stream) {
    RV_REQUIRE(tensors && chunks && partial && n_chunks > 0, "rv_adamw_step: null argument");
    RV_REQUIRE(step >= 1 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "rv_adamw_step: bad hyper-parameters");
    OptHyper h;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    h.decay = (float)(1.0 - lr * weight_decay);
    h.one_minus_beta1 = (float)(1.0 - beta1);
    h.beta2 = (float)beta2;
    h.one_minus_beta2 = (float)(1.0 - beta2);
    h.step_size = (float)(lr / bc1);
    h.bc2_sqrt = (float)sqrt(bc2);
    h.eps = (float)eps;
    h.max_norm = (float)max_norm;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(optim_sqnorm_kernel, dim3(n_chunks), dim3(256), 0, st, (const OptTensor*)tensors, (const OptChunk*)chunks, partial);
    hipLaunchKernelGGL(optim_adamw_kernel, dim3(n_chunks), dim3(256), 0, st, (const OptTensor*)tensors, (const OptChunk*)chunks, partial,
                       n_chunks, h, total_norm);
    RV_CHECK_LAUNCH("optim_adamw_kernel");
    return 0;
}

extern "C" int32_t rv_adam_max_rows(void) { return kMaxRows; }

extern "C" int rv_adamw_step_groups(const void* tensors, const int32_t* tensor_row, const void* vmax, const void* chunks, int32_t n_chunks,
                                    float* partial, const rvAdamRow* rows, int32_t n_rows, double max_norm, float* total_norm,
                                    rvStream stream) {
    RV_REQUIRE(tensors && tensor_row && chunks && partial && rows && n_chunks > 0, "rv_adamw_step_groups: null argument");
    RV_REQUIRE(n_rows >= 1 && n_rows <= kMaxRows, "rv_adamw_step_groups: n_rows = %d, outside 1 .. rv_adam_max_rows() = %d", (int)n_rows, kMaxRows);
    static_assert(sizeof(OptRows) + 64 <= 3072, "the kernel arguments must stay well under 4 KB");
    OptRows k;
    memset(&k, 0, sizeof k);
    for (int i = 0; i < n_rows; ++i) {
        const rvAdamRow& a = rows[i];
        RV_REQUIRE(a.step >= 1 && a.beta1 >= 0.0 && a.beta1 < 1.0 && a.beta2 >= 0.0 && a.beta2 < 1.0,
                   "rv_adamw_step_groups: bad hyper-parameters in row %d", i);
        RV_REQUIRE((a.flags & ~(RV_ADAM_AMSGRAD | RV_ADAM_MAXIMIZE)) == 0, "rv_adamw_step_groups: unknown flags %d in row %d", (int)a.flags, i);
        RV_REQUIRE(!(a.flags & RV_ADAM_AMSGRAD) || vmax, "rv_adamw_step_groups: row %d has RV_ADAM_AMSGRAD and vmax is null", i);
        const double bc1 = 1.0 - pow(a.beta1, (double)a.step), bc2 = 1.0 - pow(a.beta2, (double)a.step);
        OptRow& r = k.r[i];
        r.decay = (float)(1.0 - a.lr * a.weight_decay);
        r.one_minus_beta1 = (float)(1.0 - a.beta1);
        r.beta2 = (float)a.beta2;
        r.one_minus_beta2 = (float)(1.0 - a.beta2);
        r.step_size = (float)(a.lr / bc1);
        r.bc2_sqrt = (float)sqrt(bc2);
        r.eps = (float)a.eps;
        r.flags = a.flags;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(optim_sqnorm_kernel, dim3(n_chunks), dim3(256), 0, st, (const OptTensor*)tensors, (const OptChunk*)chunks, partial);
    hipLaunchKernelGGL(optim_adamw_groups_kernel, dim3(n_chunks), dim3(256), 0, st, (const OptTensor*)tensors, tensor_row,
                       (float* const*)vmax, (const OptChunk*)chunks, partial, n_chunks, (float)max_norm, n_rows, total_norm, k);
    RV_CHECK_LAUNCH("optim_adamw_groups_kernel");
    return 0;
}

// the host part of rv_adamw_step_groups: checks the rows and forms their fp32 scalars
static int adam_rows_of(const char* who, const rvAdamRow* rows, int32_t n_rows, const void* vmax, OptRows& k) {
    RV_REQUIRE(n_rows >= 1 && n_rows <= kMaxRows, "%s: n_rows = %d, outside 1 .. rv_adam_max_rows() = %d", who, (int)n_rows, kMaxRows);
    memset(&k, 0, sizeof k);
    for (int i = 0; i < n_rows; ++i) {
        const rvAdamRow& a = rows[i];
        RV_REQUIRE(a.step >= 1 && a.beta1 >= 0.0 && a.beta1 < 1.0 && a.beta2 >= 0.0 && a.beta2 < 1.0, "%s: bad hyper-parameters in row %d", who, i);
        RV_REQUIRE((a.flags & ~(RV_ADAM_AMSGRAD | RV_ADAM_MAXIMIZE)) == 0, "%s: unknown flags %d in row %d", who, (int)a.flags, i);
        RV_REQUIRE(!(a.flags & RV_ADAM_AMSGRAD) || vmax, "%s: row %d has RV_ADAM_AMSGRAD and vmax is null", who, i);
        const double bc1 = 1.0 - pow(a.beta1, (double)a.step), bc2 = 1.0 - pow(a.beta2, (double)a.step);
        OptRow& r = k.r[i];
        r.decay = (float)(1.0 - a.lr * a.weight_decay);
        r.one_minus_beta1 = (float)(1.0 - a.beta1);
        r.beta2 = (float)a.beta2;
        r.one_minus_beta2 = (float)(1.0 - a.beta2);
        r.step_size = (float)(a.lr / bc1);
        r.bc2_sqrt = (float)sqrt(bc2);
        r.eps = (float)a.eps;
        r.flags = a.flags;
    }
    return 0;
}

extern "C" int rv_adamw_step_groups_avg(const void* tensors, const int32_t* tensor_row, const void* vmax, const void* avg, double avg_weight,
                                        const void* chunks, int32_t n_chunks, float* partial, const rvAdamRow* rows, int32_t n_rows,
                                        double max_norm, float* total_norm, rvStream stream) {
    RV_REQUIRE(tensors && tensor_row && avg && chunks && partial && rows && n_chunks > 0, "rv_adamw_step_groups_avg: null argument");
    RV_REQUIRE(avg_weight >= 0.0 && avg_weight <= 1.0, "rv_adamw_step_groups_avg: avg_weight = %g, outside [0, 1]", avg_weight);
    static_assert(sizeof(OptRows) + 80 <= 3072, "the kernel arguments must stay well under 4 KB");
    OptRows k;
    if (int rc = adam_rows_of("rv_adamw_step_groups_avg", rows, n_rows, vmax, k)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(optim_sqnorm_kernel, dim3(n_chunks), dim3(256), 0, st, (const OptTensor*)tensors, (const OptChunk*)chunks, partial);
    hipLaunchKernelGGL(optim_adamw_groups_avg_kernel, dim3(n_chunks), dim3(256), 0, st, (const OptTensor*)tensors, tensor_row,
                       (float* const*)vmax, (float* const*)avg, (float)avg_weight, (const OptChunk*)chunks, partial, n_chunks,
                       (float)max_norm, n_rows, total_norm, k);
    RV_CHECK_LAUNCH("optim_adamw_groups_avg_kernel");
    return 0;
}

extern "C" int rv_average_tensors(const void* table, const void* chunks, int32_t n_chunks, double avg_weight, rvStream stream) {
    RV_REQUIRE(table && chunks, "rv_average_tensors: null argument");
    RV_REQUIRE(n_chunks > 0, "rv_average_tensors: n_chunks = %d", (int)n_chunks);
    RV_REQUIRE(avg_weight >= 0.0 && avg_weight <= 1.0, "rv_average_tensors: avg_weight = %g, outside [0, 1]", avg_weight);
    hipLaunchKernelGGL(average_tensors_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const AvgTensor*)table,
                       (const OptChunk*)chunks, (float)avg_weight);
    RV_CHECK_LAUNCH("average_tensors_kernel");
    return 0;
}
