// Global-norm gradient clipping and the Adam update (gfx950): what main.py:69-70 does every step with
// torch.nn.utils.clip_grad_norm_ and torch.optim.Adam.step, as two passes over the data —
//   (1) read every gradient once: per-tensor sums of squares (chunk partials, then a fold per tensor), (2) the clip
//   coefficient from them, (3) read g, p, m, v and write p, m, v once.
// The gradients are never written: the coefficient is applied where the update reads them. No atomics, no spinning: every
// sum has a fixed order, so the same inputs give the same bits. Pointers and lengths travel BY VALUE in the kernel arguments,
// MGCN_ADAM_BATCH tensors per launch: gradient buffers change from step to step and no device-side table outlives a call.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mgcn_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int TPB = 256;
constexpr int CHUNK = MGCN_ADAM_CHUNK;       // elements per workgroup: 8 float4 per thread
constexpr int BATCH = MGCN_ADAM_BATCH;       // tensors per launch
static_assert(CHUNK % (4 * TPB) == 0, "a chunk is whole float4 rounds of the workgroup");

// chunk0[t] .. chunk0[t + 1]: the workgroups (= chunks) of tensor t within this launch; a skipped tensor has none
struct ChunkMap {
  int32_t chunk0[BATCH + 1];
  int32_t count;
};

struct NormBatch {
  const float *g[BATCH];
  int64_t n[BATCH];
  ChunkMap map;
};

struct StepBatch {
  const float *g[BATCH];
  float *p[BATCH];
  float *m[BATCH];
  float *v[BATCH];
  int64_t n[BATCH];
  ChunkMap map;
};

struct Hyper {
  float neg_step, bc2_sqrt, omb1, b2, omb2, eps, wd;
};

// the tensor whose chunk range holds workgroup `wg` (the last t with chunk0[t] <= wg: empty ranges are stepped over)
__device__ __forceinline__ int tensor_of(const ChunkMap &map, int wg) {
  int lo = 0, hi = map.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (map.chunk0[mid] <= wg) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool dev_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// (1a) part[part0 + workgroup] = sum of squares of one chunk: per thread four chains over its float4s in ascending order,
// (c0 + c1) + (c2 + c3), then a halving tree over the workgroup. A base that is only 4-byte aligned walks scalars.
__global__ __launch_bounds__(TPB) void sq_partial_kernel(NormBatch b, float *__restrict__ part, int64_t part0) {
  __shared__ float red[TPB];
  const int wg = blockIdx.x, tid = threadIdx.x;
  const int t = tensor_of(b.map, wg);
  const int64_t e0 = int64_t(wg - b.map.chunk0[t]) * CHUNK;
  const int64_t left = b.n[t] - e0;
  const int len = left < CHUNK ? int(left) : CHUNK;
  const float *__restrict__ g = b.g[t] + e0;
  float s;
  if (dev_aligned16(g)) {
    const int nv = len >> 2;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
#pragma unroll 4
    for (int i = tid; i < nv; i += TPB) {
      const f32x4 x = reinterpret_cast<const f32x4 *>(g)[i];
      c0 += x.x * x.x;
      c1 += x.y * x.y;
      c2 += x.z * x.z;
      c3 += x.w * x.w;
    }
    s = (c0 + c1) + (c2 + c3);
    const int i = (nv << 2) + tid;             // the last len % 4 elements
    if (i < len) s += g[i] * g[i];
  } else {
    s = 0.f;
    for (int i = tid; i < len; i += TPB) s += g[i] * g[i];
  }
  red[tid] = s;
  __syncthreads();
  for (int w = TPB / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) part[part0 + wg] = red[0];
}

// sum of x[lo .. hi) by one wave, in double: lane l adds elements lo + l, lo + l + 64, ... in ascending order, then a halving
// tree over the lanes. The order is a function of the count alone.
__device__ __forceinline__ double wave_sum(const float *__restrict__ x, int64_t lo, int64_t hi) {
  double s = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 64) s += double(x[i]);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  return s;
}

// (1b) sq[sq0 + t] = the fold of tensor t's chunk partials (0 for a tensor without chunks)
__global__ __launch_bounds__(64) void sq_fold_kernel(ChunkMap map, const float *__restrict__ part, int64_t part0,
                                                     float *__restrict__ sq, int64_t sq0) {
  const int t = blockIdx.x;
  const double s = wave_sum(part, part0 + map.chunk0[t], part0 + map.chunk0[t + 1]);
  if (threadIdx.x == 0) sq[sq0 + t] = float(s);
}

// (2) total = sqrt(sum sq), coef = min(max_norm / (total + 1e-6), 1): clip_grad_norm_'s formulas (a NaN stays a NaN)
__global__ __launch_bounds__(64) void clip_coef_kernel(const float *__restrict__ sq, int64_t n, float max_norm,
                                                       float *__restrict__ out) {
  const double s = wave_sum(sq, 0, n);
  if (threadIdx.x == 0) {
    const float total = float(sqrt(s));
    const float c = max_norm / (total + 1e-6f);
    out[0] = total;
    out[1] = c > 1.0f ? 1.0f : c;
  }
}

// torch's single-tensor Adam (amsgrad = False, maximize = False), operation for operation
template <bool WD>
__device__ __forceinline__ void adam_one(float g, float &p, float &m, float &v, const Hyper &h, float coef) {
  float gc = coef * g;
  if (WD) gc = gc + h.wd * p;                        // grad.add(param, alpha = weight_decay)
  m = m + h.omb1 * (gc - m);                         // exp_avg.lerp_(grad, 1 - beta1)
  v = v * h.b2 + (h.omb2 * gc) * gc;                 // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p = p + h.neg_step * (m / denom);                  // param.addcdiv_(exp_avg, denom, value = -step_size)
}

// (3) one chunk of one tensor per workgroup: 16-byte accesses when all four bases allow it, scalars otherwise and for the
// last numel % 4 elements. g is read only. HD: the two scalars that change from step to step, step_size and bc2_sqrt, are
// loaded from hyper_dev[0 .. 2) instead of travelling in `h` (mgcn_adam_step_dev: a captured launch reads each replay's values);
// everything after the load is the same code, so the same two floats give the same bits.
template <bool WD, bool HD>
__global__ __launch_bounds__(TPB) void adam_step_kernel(StepBatch b, Hyper h, const float *__restrict__ coef_dev,
                                                        const float *__restrict__ hyper_dev) {
  const int wg = blockIdx.x, tid = threadIdx.x;
  if (HD) {
    h.neg_step = -hyper_dev[0];
    h.bc2_sqrt = hyper_dev[1];
  }
  const int t = tensor_of(b.map, wg);
  const int64_t e0 = int64_t(wg - b.map.chunk0[t]) * CHUNK;
  const int64_t left = b.n[t] - e0;
  const int len = left < CHUNK ? int(left) : CHUNK;
  const float coef = coef_dev ? *coef_dev : 1.0f;
  const float *__restrict__ g = b.g[t] + e0;
  float *__restrict__ p = b.p[t] + e0;
  float *__restrict__ m = b.m[t] + e0;
  float *__restrict__ v = b.v[t] + e0;
  int done = 0;
  if (dev_aligned16(g) && dev_aligned16(p) && dev_aligned16(m) && dev_aligned16(v)) {
    const int nv = len >> 2;
#pragma unroll 2
    for (int i = tid; i < nv; i += TPB) {
      const f32x4 gg = reinterpret_cast<const f32x4 *>(g)[i];
      f32x4 pp = reinterpret_cast<f32x4 *>(p)[i];
      f32x4 mm = reinterpret_cast<f32x4 *>(m)[i];
      f32x4 vv = reinterpret_cast<f32x4 *>(v)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float p1 = pp[k], m1 = mm[k], v1 = vv[k];
        adam_one<WD>(gg[k], p1, m1, v1, h, coef);
        pp[k] = p1;
        mm[k] = m1;
        vv[k] = v1;
      }
      reinterpret_cast<f32x4 *>(p)[i] = pp;
      reinterpret_cast<f32x4 *>(m)[i] = mm;
      reinterpret_cast<f32x4 *>(v)[i] = vv;
    }
    done = nv << 2;
  }
  for (int i = done + tid; i < len; i += TPB) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam_one<WD>(g[i], pp, mm, vv, h, coef);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
  }
}

inline int64_t chunks_of(int64_t numel) { return (numel + CHUNK - 1) / CHUNK; }

// n >= 0, the arrays present, no negative length
int check_list(const char *what, int64_t n, const void *first_array, const int64_t *numel_host) {
  MGCN_REQUIRE(n >= 0, "%s: bad sizes (n = %lld)", what, (long long)n);
  MGCN_REQUIRE(n == 0 || (first_array && numel_host), "%s: null pointer (host array)", what);
  for (int64_t i = 0; i < n; ++i)
    MGCN_REQUIRE(numel_host[i] >= 0, "%s: bad sizes (tensor %lld has %lld elements)", what, (long long)i, (long long)numel_host[i]);
  return MGCN_OK;
}

}  // namespace

extern "C" size_t mgcn_adam_sq_norms_workspace(int64_t n, const int64_t *numel_host) {
  if (n < 0 || (n > 0 && !numel_host)) return 0;
  int64_t chunks = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (numel_host[i] < 0) return 0;
    chunks += chunks_of(numel_host[i]);
  }
  return size_t(chunks) * sizeof(float);
}

extern "C" int mgcn_adam_sq_norms(int64_t n, const float *const *grad_host, const int64_t *numel_host, float *sq_dev,
                                  void *workspace_dev, size_t workspace_bytes, void *stream) {
  if (int rc = check_list("mgcn_adam_sq_norms", n, grad_host, numel_host)) return rc;
  MGCN_REQUIRE(n == 0 || sq_dev, "mgcn_adam_sq_norms: null pointer (sq)");
  const size_t need = mgcn_adam_sq_norms_workspace(n, numel_host);
  MGCN_REQUIRE(workspace_bytes >= need, "mgcn_adam_sq_norms: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
  MGCN_REQUIRE(need == 0 || (workspace_dev && (reinterpret_cast<uintptr_t>(workspace_dev) & 3u) == 0),
               "mgcn_adam_sq_norms: null pointer or misaligned workspace");
  for (int64_t i0 = 0; i0 < n; i0 += BATCH)        // every launch's grid fits: checked before the first one
    for (int64_t i = i0, c = 0; i < n && i < i0 + BATCH; ++i) {
      c += chunks_of(numel_host[i]);
      if (c > INT32_MAX) return mgcn::fail(MGCN_EUNSUPPORTED, "mgcn_adam_sq_norms: more than 2^31 chunks in one launch");
    }
  float *part = static_cast<float *>(workspace_dev);
  int64_t part0 = 0;
  for (int64_t i0 = 0; i0 < n; i0 += BATCH) {
    NormBatch b;
    const int count = int(n - i0 < BATCH ? n - i0 : BATCH);
    int32_t c = 0;
    int64_t reserved = 0;
    for (int t = 0; t < BATCH; ++t) {
      const bool live = t < count && grad_host[i0 + t] && numel_host[i0 + t] > 0;
      b.g[t] = live ? grad_host[i0 + t] : nullptr;
      b.n[t] = live ? numel_host[i0 + t] : 0;
      b.map.chunk0[t] = c;
      if (live) c += int32_t(chunks_of(numel_host[i0 + t]));
      if (t < count) reserved += chunks_of(numel_host[i0 + t]);
    }
    b.map.chunk0[BATCH] = c;
    b.map.count = count;
    if (c > 0) {
      sq_partial_kernel<<<dim3(c), dim3(TPB), 0, static_cast<hipStream_t>(stream)>>>(b, part, part0);
      MGCN_CHECK_LAUNCH("mgcn_adam_sq_norms (partials)");
    }
    sq_fold_kernel<<<dim3(count), dim3(64), 0, static_cast<hipStream_t>(stream)>>>(b.map, part, part0, sq_dev, i0);
    MGCN_CHECK_LAUNCH("mgcn_adam_sq_norms (fold)");
    part0 += reserved;
  }
  return MGCN_OK;
}

extern "C" int mgcn_adam_clip_coef(int64_t n, const float *sq_dev, float max_norm, float *out_dev, void *stream) {
  MGCN_REQUIRE(n >= 0, "mgcn_adam_clip_coef: bad sizes (n = %lld)", (long long)n);
  MGCN_REQUIRE((n == 0 || sq_dev) && out_dev, "mgcn_adam_clip_coef: null pointer");
  MGCN_REQUIRE(max_norm >= 0.f, "mgcn_adam_clip_coef: max_norm must be a number >= 0");
  clip_coef_kernel<<<dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream)>>>(sq_dev, n, max_norm, out_dev);
  MGCN_CHECK_LAUNCH("mgcn_adam_clip_coef");
  return MGCN_OK;
}

namespace {

// both forms of kernel (3). hyper_dev == nullptr: step_size and bc2_sqrt by value (mgcn_adam_step); otherwise they are read on
// the device and the two by-value arguments are not used (mgcn_adam_step_dev).
int adam_step_launch(const char *what, int64_t n, const float *const *grad_host, float *const *param_host, float *const *exp_avg_host,
                     float *const *exp_avg_sq_host, const int64_t *numel_host, const float *coef_dev, const float *hyper_dev,
                     float step_size, float bc2_sqrt, double beta1, double beta2, double eps, double weight_decay, void *stream) {
  if (int rc = check_list(what, n, grad_host, numel_host)) return rc;
  MGCN_REQUIRE(n == 0 || (param_host && exp_avg_host && exp_avg_sq_host), "%s: null pointer (host array)", what);
  MGCN_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas must lie in [0, 1)", what);
  MGCN_REQUIRE(eps >= 0.0 && weight_decay >= 0.0, "%s: eps and weight_decay must be numbers >= 0", what);
  if (!hyper_dev) {                                   // by value: checked here, in the order mgcn_adam_step has always checked
    MGCN_REQUIRE(step_size >= 0.f && std::isfinite(step_size), "%s: step_size (lr / (1 - beta1^t)) must be a finite number >= 0", what);
    MGCN_REQUIRE(bc2_sqrt > 0.f && bc2_sqrt <= 1.f, "%s: bc2_sqrt (sqrt(1 - beta2^t)) must lie in (0, 1]", what);
  }
  int64_t live = 0;
  for (int64_t i = 0, c = 0; i < n; ++i) {
    if (!grad_host[i] || numel_host[i] == 0) continue;
    MGCN_REQUIRE(param_host[i] && exp_avg_host[i] && exp_avg_sq_host[i], "%s: null pointer (tensor %lld)", what, (long long)i);
    if (live % BATCH == 0) c = 0;
    c += chunks_of(numel_host[i]);
    if (c > INT32_MAX) return mgcn::fail(MGCN_EUNSUPPORTED, "%s: more than 2^31 chunks in one launch", what);
    ++live;
  }
  Hyper h;
  h.neg_step = -step_size;                            // (both overwritten on the device when hyper_dev is given)
  h.bc2_sqrt = bc2_sqrt;
  h.omb1 = float(1.0 - beta1);
  h.b2 = float(beta2);
  h.omb2 = float(1.0 - beta2);
  h.eps = float(eps);
  h.wd = float(weight_decay);
  int64_t i = 0;
  while (live > 0) {                                  // the live tensors, BATCH per launch, in list order
    StepBatch b;
    int count = 0;
    int32_t c = 0;
    for (; i < n && count < BATCH; ++i) {
      if (!grad_host[i] || numel_host[i] == 0) continue;
      b.g[count] = grad_host[i];
      b.p[count] = param_host[i];
      b.m[count] = exp_avg_host[i];
      b.v[count] = exp_avg_sq_host[i];
      b.n[count] = numel_host[i];
      b.map.chunk0[count] = c;
      c += int32_t(chunks_of(numel_host[i]));
      ++count;
    }
    for (int t = count; t < BATCH; ++t) {
      b.g[t] = nullptr;
      b.p[t] = b.m[t] = b.v[t] = nullptr;
      b.n[t] = 0;
      b.map.chunk0[t] = c;
    }
    b.map.chunk0[BATCH] = c;
    b.map.count = count;
    live -= count;
    const dim3 grid(c), block(TPB);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hyper_dev) {
      if (h.wd != 0.f)
        adam_step_kernel<true, true><<<grid, block, 0, st>>>(b, h, coef_dev, hyper_dev);
      else
        adam_step_kernel<false, true><<<grid, block, 0, st>>>(b, h, coef_dev, hyper_dev);
    } else {
      if (h.wd != 0.f)
        adam_step_kernel<true, false><<<grid, block, 0, st>>>(b, h, coef_dev, nullptr);
      else
        adam_step_kernel<false, false><<<grid, block, 0, st>>>(b, h, coef_dev, nullptr);
    }
    MGCN_CHECK_LAUNCH(what);
  }
  return MGCN_OK;
}

}  // namespace

extern "C" int mgcn_adam_step(int64_t n, const float *const *grad_host, float *const *param_host, float *const *exp_avg_host,
                              float *const *exp_avg_sq_host, const int64_t *numel_host, const float *coef_dev, float step_size,
                              float bc2_sqrt, double beta1, double beta2, double eps, double weight_decay, void *stream) {
  return adam_step_launch("mgcn_adam_step", n, grad_host, param_host, exp_avg_host, exp_avg_sq_host, numel_host, coef_dev, nullptr,
                          step_size, bc2_sqrt, beta1, beta2, eps, weight_decay, stream);
}

extern "C" int mgcn_adam_step_dev(int64_t n, const float *const *grad_host, float *const *param_host, float *const *exp_avg_host,
                                  float *const *exp_avg_sq_host, const int64_t *numel_host, const float *coef_dev,
                                  const float *hyper_dev, double beta1, double beta2, double eps, double weight_decay, void *stream) {
  MGCN_REQUIRE(hyper_dev && (reinterpret_cast<uintptr_t>(hyper_dev) & 3u) == 0,
               "mgcn_adam_step_dev: null or misaligned pointer (hyper: two floats, step_size and bc2_sqrt)");
  return adam_step_launch("mgcn_adam_step_dev", n, grad_host, param_host, exp_avg_host, exp_avg_sq_host, numel_host, coef_dev, hyper_dev,
                          0.f, 1.f, beta1, beta2, eps, weight_decay, stream);
}
