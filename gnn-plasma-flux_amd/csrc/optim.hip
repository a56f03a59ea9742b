// The optimizer step over one flat parameter buffer (include/hybridflux.h,
// hf_adam_flat / hf_adam_flat_ex).
//
// adam_flat_kernel<false> is torch.optim.Adam's update (no weight decay, no
// amsgrad; the arithmetic of torch's fused Adam functor): the training step's
// optimizer (train_ablation.py:208-209) in one launch wide enough to stream the
// buffer, instead of a multi-tensor launch of a few workgroups.  The step count
// lives on the device (capturable): every workgroup reads it first, and the
// last workgroup to finish (a done-counter it resets) stores the incremented
// count.
//
// adam_flat_kernel<true> is the guarded step: the same per-value update
// (adam_value, the one statement of the arithmetic) behind gradient clipping by
// the global L2 norm, decoupled weight decay, a learning rate read from device
// memory and the skip of a step whose gradient norm is not finite.  The norm
// comes from a launch of its own (grad_sumsq_kernel: float64 partial sums, one
// per workgroup, over the update's own partition); every workgroup of the
// update then adds the partials in one fixed order, so all of them hold the
// same norm, clip coefficient and skip decision without a grid barrier.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "hf_internal.h"

namespace hf {

constexpr int kOptThreads = 256;     // threads of a workgroup, both kernels
constexpr int kOptTile = 1024;       // values per workgroup and grid pass the grid is sized for
constexpr int kOptMaxBlocks = 2048;  // workgroups at most: beyond kOptMaxBlocks * kOptTile values they stride

static int64_t opt_blocks(int64_t n) {
  const int64_t tiles = n / kOptTile + (n % kOptTile != 0);
  return std::min<int64_t>(std::max<int64_t>(tiles, 1), kOptMaxBlocks);
}

int64_t adam_flat_ws_bytes(int64_t n) { return opt_blocks(n) * (int64_t)sizeof(double); }

// The sum of sh[0..kOptThreads) in a fixed tree order, returned to every thread.
__device__ inline double block_sum(double *sh, double a) {
  const int t = threadIdx.x;
  sh[t] = a;
  __syncthreads();
  for (int w = kOptThreads / 2; w > 0; w >>= 1) {
    if (t < w) sh[t] = sh[t] + sh[t + w];
    __syncthreads();
  }
  return sh[0];
}

// parts[b] = sum of g[i]^2 in float64 over the values workgroup b of the update
// owns (i = b * 256 + t + k * gridDim * 256): thread t adds its values in
// ascending k, then the tree of block_sum.  The squares are formed in float64,
// so values near 1e30 do not overflow and a 1e4 beside a million 1e-4s is kept.
__global__ __launch_bounds__(kOptThreads) void grad_sumsq_kernel(const float *__restrict__ g, int64_t n,
                                                                 double *__restrict__ parts) {
  __shared__ double sh[kOptThreads];
  double a = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kOptThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kOptThreads) {
    const double gi = (double)g[i];
    a = a + gi * gi;
  }
  const double sum = block_sum(sh, a);
  if (threadIdx.x == 0) parts[blockIdx.x] = sum;
}

// What the guarded step adds to the plain one.
struct OptGuard {
  const float *lr;      // device learning rate, or NULL: the by-value one
  float wd;             // decoupled weight decay
  float max_norm;       // clip threshold (INFINITY: none)
  int skip;             // skip the step on a non-finite norm
  const double *parts;  // grad_sumsq_kernel's partials, or NULL: no norm (coef 1, never skipped)
  int nparts;
  float *stats;         // [HF_OPT_NUM_STATS] or NULL
};

// One value of Adam: m = b1 m + c1 g, v = b2 v + c2 g^2, p -= step_size m / (sqrt(v) / bc2s + eps).
__device__ inline void adam_value(float *__restrict__ p, float *__restrict__ m, float *__restrict__ v, int64_t i,
                                  float pi, float gi, float b1, float b2, float c1, float c2, float step_size,
                                  float bc2s, float eps) {
  const float mi = b1 * m[i] + c1 * gi;
  const float vi = b2 * v[i] + c2 * gi * gi;
  m[i] = mi;
  v[i] = vi;
  const float denom = sqrtf(vi) / bc2s + eps;
  p[i] = pi - step_size * mi / denom;
}

template <bool GUARD>
__global__ __launch_bounds__(kOptThreads) void adam_flat_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                                float *__restrict__ m, float *__restrict__ v,
                                                                int64_t n, float *step, unsigned *done, float lr,
                                                                float b1, float b2, float eps, OptGuard q) {
  float norm = 0.0f, coef = 1.0f;
  bool skipped = false;
  if constexpr (GUARD) {
    if (q.lr) lr = q.lr[0];
    if (q.parts) {
      __shared__ double sh[kOptThreads];
      double a = 0.0;
      for (int j = threadIdx.x; j < q.nparts; j += kOptThreads) a = a + q.parts[j];
      norm = (float)sqrt(block_sum(sh, a));
      const float c = q.max_norm / (norm + 1e-6f);  // clip_grad_norm_'s coefficient, clamped at 1
      coef = c < 1.0f ? c : 1.0f;
      skipped = q.skip && !(fabsf(norm) <= 3.402823466e+38f);
    }
  }
  const float s = step[0] + 1.0f;
  if (!skipped) {
    const float bc1 = (float)(1.0 - pow((double)b1, (double)s));
    const float bc2s = (float)sqrt(1.0 - pow((double)b2, (double)s));
    const float step_size = lr / bc1, c1 = 1.0f - b1, c2 = 1.0f - b2;
    const bool clip = GUARD && coef != 1.0f, decay = GUARD && q.wd != 0.0f;
    const float keep = 1.0f - lr * q.wd;
    for (int64_t i = (int64_t)blockIdx.x * kOptThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kOptThreads) {
      float gi = g[i], pi = p[i];
      if (clip) gi = gi * coef;
      if (decay) pi = pi * keep;
      adam_value(p, m, v, i, pi, gi, b1, b2, c1, c2, step_size, bc2s, eps);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(done, 1u) == gridDim.x - 1) {
      if (!skipped) step[0] = s;
      done[0] = 0u;
      if (GUARD && q.stats) {
        q.stats[0] = norm;
        q.stats[1] = skipped ? 0.0f : coef;
        q.stats[2] = skipped ? 1.0f : 0.0f;
        q.stats[3] = q.stats[3] + (skipped ? 1.0f : 0.0f);
      }
      __threadfence();
    }
  }
}

hipError_t launch_adam_flat(float *p, const float *g, float *m, float *v, int64_t n, float *step, unsigned *done,
                            float lr, float b1, float b2, float eps, hipStream_t s) {
  hipLaunchKernelGGL(adam_flat_kernel<false>, dim3((unsigned)opt_blocks(n)), dim3(kOptThreads), 0, s, p, g, m, v, n,
                     step, done, lr, b1, b2, eps, OptGuard{});
  return hipGetLastError();
}

hipError_t launch_adam_flat_ex(float *p, const float *g, float *m, float *v, int64_t n, float *step, unsigned *done,
                               const float *dev_lr, float lr, float b1, float b2, float eps, float wd, float max_norm,
                               int skip, void *ws, float *stats, hipStream_t s) {
  const unsigned blocks = (unsigned)opt_blocks(n);
  double *parts = static_cast<double *>(ws);
  if (parts) {
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(kOptThreads), 0, s, g, n, parts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(adam_flat_kernel<true>, dim3(blocks), dim3(kOptThreads), 0, s, p, g, m, v, n, step, done, lr, b1,
                     b2, eps, OptGuard{dev_lr, wd, max_norm, skip, parts, (int)blocks, stats});
  return hipGetLastError();
}

}  // namespace hf
