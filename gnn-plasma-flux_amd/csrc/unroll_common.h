// What the unrolled-training kernels (unroll.hip, pure_unroll.hip,
// pinn_unroll.hip) and pinn_train.hip's loss share: the float64 wave sum, the
// squared-error term, the last-arriver ticket, the energy / charge coefficient
// formula, and the state-loss arguments of the two update launchers with their
// host-side fill.  The ticket's memory ordering and the conservation formula
// exist here and nowhere else.
#pragma once
#include "hf_internal.h"

namespace hf {
namespace {

// Every workspace starts with the arrival counter: [0, 256), zeroed by the
// launcher's memset node before every launch; the float64 loss partials
// follow, and behind them the conservation terms' partials of an _ex call.
constexpr size_t kCounterBytes = 256;
struct LossWs {
  unsigned *cnt;
  double *part, *cons_part;
  size_t bytes;
};
inline LossWs carve_loss_ws(size_t parts, size_t cons_parts, void *base) {
  Carve c(base);
  LossWs w{};
  w.cnt = reinterpret_cast<unsigned *>(c.take<char>(kCounterBytes));
  w.part = c.take<double>(parts);
  w.cons_part = c.take<double>(cons_parts);
  w.bytes = c.off;
  return w;
}

__device__ __forceinline__ double wave_sum(double a) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
  return a;
}

// w (pred - target)^2 of one value, the difference rounded to float32
__device__ __forceinline__ double sq_err(float pred, float tgt, float w) {
  const double d = (double)__fsub_rn(pred, tgt);
  return (double)w * (d * d);
}

// The last-arriver ticket of a launch whose waves each store partials and then,
// whole, run
//   if (arrival_ticket(cnt, lane) != total - 1) return;
//   acquire_partials();
// `total` the number of waves that do: only the wave that arrives last goes
// on, and it may read every wave's partials.  Agent-scope release before the
// ticket, agent-scope acquire after the last one (the per-XCD L2s are not
// coherent).  The comparison stays with the caller, which keeps its branch (and
// where it reads gridDim.x) as the kernels always had them.
__device__ __forceinline__ unsigned arrival_ticket(unsigned *cnt, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  unsigned t = 0;
  if (lane == 0) t = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __shfl(t, 0, 64);
}
__device__ __forceinline__ void acquire_partials() {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The state-loss and conservation arguments of the FluxGNN and PureGNN update
// kernels.  Each file derives its LossArgs / ConsArgs from these, so the
// kernels' parameter types keep their names (and PureGNN's ConsArgs its tail);
// pinn_unroll.hip's own LossArgs holds a StateConsArgs.
struct StateLossArgs {
  const float *tgt;  // [B][3][nx] or NULL: no loss term
  float w0, w1, w2;
  double scale;
  double *part;      // one per partial-writing wave, behind the counter
  unsigned *cnt;
  float *loss;
};
// The energy and charge terms of the _ex calls: on == false leaves the kernel
// with the state term alone and the wider loss row.
struct StateConsArgs {
  bool on;
  double lam_e, lam_q, scale;  // scale = cons_scale
  const double *ref;           // [B][2] (eref, qref)
  float *coef;                 // [B][2] (ce, cq)
  double *part;                // the terms' partials (LossWs::cons_part)
};

// The energy and charge terms of IC b (include/hybridflux.h) from its complete
// sums: r_e = 0.5 (sum u^2 + sum E^2) / nx - eref, r_q = sum n / nx - qref.
// Writes the adjoint's coefficients (ce, cq) = 2 lam s r / nx of the IC and its
// term partials (pe, pq) = lam r^2, which a caller stores or adds up.
// Everything in float64, the coefficients rounded once.  NX: int, or double
// for a caller that holds nx converted.
template <class I, class NX>
__device__ __forceinline__ void cons_terms(const StateConsArgs &ca, I b, double su2, double sE2, double sn, NX nx,
                                           double &pe, double &pq) {
  const double re = 0.5 * (su2 + sE2) / (double)nx - ca.ref[2 * b], rq = sn / (double)nx - ca.ref[2 * b + 1];
  ca.coef[2 * b] = (float)(2.0 * ca.lam_e * ca.scale * re / (double)nx);
  ca.coef[2 * b + 1] = (float)(2.0 * ca.lam_q * ca.scale * rq / (double)nx);
  pe = ca.lam_e * (re * re);
  pq = ca.lam_q * (rq * rq);
}

// Turns the terms on.
inline void cons_setup(StateConsArgs &ca, const ConsTerms &cons, double *cons_part) {
  ca.on = true;
  ca.lam_e = (double)cons.lam_e, ca.lam_q = (double)cons.lam_q, ca.scale = (double)cons.scale;
  ca.ref = cons.ref, ca.coef = cons.coef;
  ca.part = cons_part;
}

// Fills both for a launch with a target (cons NULL: the terms stay off) and
// enqueues the counter's reset.
inline hipError_t state_loss_setup(StateLossArgs &la, StateConsArgs &ca, const float *target, const float *w,
                                   float scale, float *loss, const LossWs &ws, const ConsTerms *cons, hipStream_t s) {
  la.tgt = target;
  la.w0 = w[0], la.w1 = w[1], la.w2 = w[2];
  la.scale = (double)scale;
  la.cnt = ws.cnt;
  la.part = ws.part;
  la.loss = loss;
  if (cons) cons_setup(ca, *cons, ws.cons_part);
  // the arrival counter starts every launch at 0 (a memset node, not a kernel)
  return hipMemsetAsync(ws.cnt, 0, 16, s);
}

}  // namespace
}  // namespace hf
