// Unrolled training of PINN: the loss term of one rollout step
// (hf_pinn_unroll_loss) and the gradient that step's hf_pinn_backward takes in
// (hf_pinn_unroll_adjoint), one launch each (scripts/evaluation/
// evaluate_multi_ic.py:70-83 under a K-step loss; include/hybridflux.h has the
// mathematics).
//
// Both kernels: one 256-thread workgroup per IC, thread t owns cells t, t +
// 256, ... in every phase.  Residuals and sums in float64.  The circulant
// column of the spectral Poisson operator P (double), p_n - 1 and r~ live in
// LDS (16 nx bytes, pinn_loss_kernel's budget: nx <= kFvLdsMaxNx); the adjoint
// reuses those bytes for q_c and q_m of the following step once P is done.
//
// The loss follows pure_unroll.hip term for term (the float32 difference,
// squared and weighted in float64, a cell's three channels added first), so
// with phys == NULL and nx <= 1024 (one tile of that kernel per IC) it gives
// hf_pure_unroll_update's loss bit for bit; beyond 1024 cells the partials are
// cut differently.  Per-IC float64 partials, summed in IC order by the last
// workgroup to arrive (pinn_loss_kernel's scheme).  No float atomics; every
// output value is written by one thread in a fixed order.
#include "hf_device.h"
#include "hf_internal.h"
#include "unroll_common.h"

namespace hf {
namespace {

constexpr int kPuThreads = 256;
// Workspace: [0, kCounterBytes) the arrival counter, then four float64
// partials per IC (data, cont, mom, pois); the _ex call with the conservation
// terms adds two per IC behind them (lam_e r_e^2, lam_q r_q^2).  The data
// term is pure_unroll.hip's (sq_err).

// The residuals' constants; phys == false: only the data term.
struct Phys {
  bool on, pois;         // pois: lambda_p != 0 (else no O(nx^2) work)
  const float *s;        // the state slot (n, u, E) [B][3][nx]
  const double *pc;      // the circulant column, plan[0..nx)
  double inv_dt, inv_2dx, nu_dx2;
};

// r_c and r_m of cell i: p = (pn, pu) the prediction, S the state slot's rows of this IC
__device__ __forceinline__ void residuals(const float *S, int i, int nx, double pn, double pu, const Phys &f,
                                          double &rc, double &rm) {
  const int ip = i == nx - 1 ? 0 : i + 1, im = i == 0 ? nx - 1 : i - 1;
  const double n = S[i], u = S[nx + i], E = S[2 * nx + i];
  const double up = S[nx + ip], um = S[nx + im];
  rc = (pn - n) * f.inv_dt + ((double)S[ip] * up - (double)S[im] * um) * f.inv_2dx;
  rm = (pu - u) * f.inv_dt + u * (up - um) * f.inv_2dx + E - f.nu_dx2 * (up - 2.0 * u + um);
}

// ------------------------------------------------------------------------ loss
struct LossArgs {
  const float *p, *t;  // pred, target [B][3][nx]
  Phys f;
  int B, nx;
  float w0, w1, w2;
  double scale;         // loss_scale
  double sc, sm, sp;    // phys_scale * lambda_c, _m, _p
  double *part;         // [B][4]
  unsigned *cnt;
  float *losses;
  StateConsArgs c;      // the _ex call's energy and charge terms, part [B][2]; off: the wider row only
};

template <bool EX>
__global__ __launch_bounds__(kPuThreads) void pinn_unroll_loss_kernel(LossArgs a) {
  extern __shared__ double s_dyn[];
  __shared__ double red[4][4];
  const int nx = a.nx;
  double *Lc = s_dyn;  // (used with f.pois only)
  float *Lrho = reinterpret_cast<float *>(Lc + nx);
  const int64_t b = blockIdx.x;
  const float *P = a.p + b * 3 * nx, *T = a.t + b * 3 * nx;
  const float *S = a.f.on ? a.f.s + b * 3 * nx : nullptr;
  if (a.f.pois) {  // (uniform)
    for (int i = threadIdx.x; i < nx; i += kPuThreads) {
      Lc[i] = a.f.pc[i];
      Lrho[i] = __fsub_rn(P[i], 1.0f);  // P has zero row sums: P p_n = P (p_n - 1), the solver's operand
    }
    __syncthreads();
  }
  const bool cons = EX && a.c.on;
  double sd = 0.0, sc = 0.0, sm = 0.0, sp = 0.0, su2 = 0.0, sE2 = 0.0, sn = 0.0;
  for (int i = threadIdx.x; i < nx; i += kPuThreads) {
    const float pn = P[i], pu = P[nx + i], pE = P[2 * nx + i];
    sd += sq_err(pn, T[i], a.w0) + sq_err(pu, T[nx + i], a.w1) + sq_err(pE, T[2 * nx + i], a.w2);
    if (cons) {
      su2 += (double)pu * (double)pu;
      sE2 += (double)pE * (double)pE;
      sn += (double)pn;
    }
    if (a.f.on) {
      double rc, rm;
      residuals(S, i, nx, pn, pu, a.f, rc, rm);
      sc += rc * rc;
      sm += rm * rm;
      if (a.f.pois) {
        // X[0] = 0, X[i] = -(P p_n)[i] (train_pinn.py:72-74)
        const double X = i == 0 ? 0.0 : -(double)poisson_cell(Lrho, Lc, i, nx);
        const double rp = (double)pE - X;
        sp += rp * rp;
      }
    }
  }
  sd = wave_sum(sd);
  sc = wave_sum(sc);
  sm = wave_sum(sm);
  sp = wave_sum(sp);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave][0] = sd, red[wave][1] = sc, red[wave][2] = sm, red[wave][3] = sp;
  if constexpr (EX) {
    __shared__ double redc[4][3];
    if (cons) {  // (uniform)
      su2 = wave_sum(su2);
      sE2 = wave_sum(sE2);
      sn = wave_sum(sn);
      if (lane == 0) redc[wave][0] = su2, redc[wave][1] = sE2, redc[wave][2] = sn;
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    if (cons && lane == 0) {
      // this IC's complete sums: its coefficients (float64, rounded once) and its two term partials
      const double tu = ((redc[0][0] + redc[1][0]) + redc[2][0]) + redc[3][0];
      const double tE = ((redc[0][1] + redc[1][1]) + redc[2][1]) + redc[3][1];
      const double tn = ((redc[0][2] + redc[1][2]) + redc[2][2]) + redc[3][2];
      double pe, pq;
      cons_terms(a.c, b, tu, tE, tn, nx, pe, pq);
      a.c.part[2 * b] = pe;
      a.c.part[2 * b + 1] = pq;
    }
  } else {
    __syncthreads();
    if (threadIdx.x >= 64) return;
  }
  if (lane < 4) a.part[b * 4 + lane] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
  // The last workgroup to arrive sums the partials.  Each lane sums its ICs in
  // ascending order, then the lanes in a fixed tree: the value does not depend
  // on which workgroup arrives last.
  if (arrival_ticket(a.cnt, lane) != gridDim.x - 1) return;
  acquire_partials();
  double q[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = lane; i < a.B; i += 64) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] += a.part[(int64_t)i * 4 + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = wave_sum(q[k]);
  double qe = 0.0, qq = 0.0;
  if (cons) {  // (uniform)
    for (int i = lane; i < a.B; i += 64) qe += a.c.part[2 * (int64_t)i], qq += a.c.part[2 * (int64_t)i + 1];
    qe = wave_sum(qe);
    qq = wave_sum(qq);
  }
  if (lane == 0) {
    const double ld = q[0] * a.scale, lc = q[1] * a.sc, lm = q[2] * a.sm, lp = q[3] * a.sp;
    if constexpr (EX) {
      // (total, data, cont, mom, pois, energy, charge): entries 1..4 are the plain call's, and so is 0 without the terms
      const double le = qe * a.c.scale, lq = qq * a.c.scale;
      a.losses[0] = cons ? (float)(((((ld + lc) + lm) + lp) + le) + lq) : (float)(((ld + lc) + lm) + lp);
      a.losses[1] = (float)ld;
      a.losses[2] = (float)lc;
      a.losses[3] = (float)lm;
      a.losses[4] = (float)lp;
      a.losses[5] = (float)le;
      a.losses[6] = (float)lq;
      return;
    }
    a.losses[0] = (float)(((ld + lc) + lm) + lp);
    a.losses[1] = (float)ld;
    a.losses[2] = (float)lc;
    a.losses[3] = (float)lm;
    a.losses[4] = (float)lp;
  }
}

// --------------------------------------------------------------------- adjoint
struct AdjArgs {
  const float *p, *t;  // pred = s^_k, target = s*_k [B][3][nx]
  Phys f;              // f.s = s^_{k-1}
  const float *pnext;  // s^_{k+1} or NULL (read with f.on only)
  const float *carry;  // hf_pinn_backward's dL/dstate of step k+1, or NULL
  int nx;
  double gd0, gd1, gd2;  // 2 w_ch loss_scale
  double gc, gm, gp;     // 2 phys_scale lambda_c / dt, ... lambda_m / dt, ... lambda_p
  double qc, qm;         // 2 phys_scale lambda_c, ... lambda_m
  float *g;
  const float *coef;     // [B][2] = (ce, cq) or NULL (read by the EX kernel only)
};

// EX with coef: d term_k / d p gains cq_b, ce_b p_u, ce_b p_E on its three
// channels (one float32 product; added to the state seed before the residual terms).
template <bool EX>
__global__ __launch_bounds__(kPuThreads) void pinn_unroll_adjoint_kernel(AdjArgs a) {
  extern __shared__ double s_dyn[];
  const int nx = a.nx;
  const int64_t b = blockIdx.x;
  const float *P = a.p + b * 3 * nx, *T = a.t + b * 3 * nx;
  const float *S = a.f.on ? a.f.s + b * 3 * nx : nullptr;
  float *G = a.g + b * 3 * nx;
  // ---- part 1: d term_k / d p, hf_pinn_loss's dL/dp
  double *Lc = s_dyn;
  float *Lrho = reinterpret_cast<float *>(Lc + nx), *Lrt = Lrho + nx;
  if (a.f.pois) {  // (uniform)
    for (int i = threadIdx.x; i < nx; i += kPuThreads) {
      Lc[i] = a.f.pc[i];
      Lrho[i] = __fsub_rn(P[i], 1.0f);
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < nx; i += kPuThreads) {
    const double pn = P[i], pu = P[nx + i], pE = P[2 * nx + i];
    double gn = a.gd0 * (pn - (double)T[i]), gu = a.gd1 * (pu - (double)T[nx + i]),
           gE = a.gd2 * (pE - (double)T[2 * nx + i]);
    if constexpr (EX) {
      if (a.coef) {  // (uniform)
        const float ce = a.coef[2 * b];
        gn += (double)a.coef[2 * b + 1];
        gu += (double)(ce * P[nx + i]);
        gE += (double)(ce * P[2 * nx + i]);
      }
    }
    if (a.f.on) {
      double rc, rm;
      residuals(S, i, nx, pn, pu, a.f, rc, rm);
      gn += a.gc * rc;  // the P r~ term is added below
      gu += a.gm * rm;
      if (a.f.pois) {
        const double X = i == 0 ? 0.0 : -(double)poisson_cell(Lrho, Lc, i, nx);
        const double rp = pE - X;
        Lrt[i] = i == 0 ? 0.f : (float)rp;  // r~ = r_p with cell 0 zeroed
        gE += a.gp * rp;
      }
    }
    G[i] = (float)gn;
    G[nx + i] = (float)gu;
    G[2 * nx + i] = (float)gE;
  }
  if (a.f.pois) {
    __syncthreads();
    // dL/dp_n -= 2 phys_scale lambda_p (P r~)   (P^T = -P; this thread's own store above)
    for (int i = threadIdx.x; i < nx; i += kPuThreads)
      G[i] = (float)((double)G[i] - a.gp * (double)poisson_cell(Lrt, Lc, i, nx));
  }
  const bool back = a.f.on && a.pnext;  // part 2 is present
  if (!back && !a.carry) return;          // (uniform)
  // ---- part 2: d term_{k+1} / d (state slot), residuals of step k+1 with p' =
  // s^_{k+1} and (n, u, E) = s^_k; q_c, q_m over the bytes P no longer needs
  double *Lqc = s_dyn, *Lqm = s_dyn + nx;
  if (back) {
    const float *N = a.pnext + b * 3 * nx;
    __syncthreads();
    for (int i = threadIdx.x; i < nx; i += kPuThreads) {
      double rc, rm;
      residuals(P, i, nx, (double)N[i], (double)N[nx + i], a.f, rc, rm);
      Lqc[i] = a.qc * rc;
      Lqm[i] = a.qm * rm;
    }
    __syncthreads();
  }
  // ---- the sum: (part 1 + part 2) + part 3, this thread's own stores above
  const float *C = a.carry ? a.carry + b * 3 * nx : nullptr;
  for (int i = threadIdx.x; i < nx; i += kPuThreads) {
    double gn = G[i], gu = G[nx + i], gE = G[2 * nx + i];
    if (back) {
      const int ip = i == nx - 1 ? 0 : i + 1, im = i == 0 ? nx - 1 : i - 1;
      const double n = P[i], u = P[nx + i], up = P[nx + ip], um = P[nx + im];
      const double dqc = (Lqc[im] - Lqc[ip]) * a.f.inv_2dx;
      gn += -Lqc[i] * a.f.inv_dt + u * dqc;
      gu += ((n * dqc + Lqm[i] * (-a.f.inv_dt + (up - um) * a.f.inv_2dx + 2.0 * a.f.nu_dx2)) +
             Lqm[im] * (um * a.f.inv_2dx - a.f.nu_dx2)) +
            Lqm[ip] * (-up * a.f.inv_2dx - a.f.nu_dx2);
      gE += Lqm[i];
    }
    if (C) gn += (double)C[i], gu += (double)C[nx + i], gE += (double)C[2 * nx + i];
    G[i] = (float)gn;
    G[nx + i] = (float)gu;
    G[2 * nx + i] = (float)gE;
  }
}

Phys phys_of(const float *state, const float *phys, double dt, double dx, double nu, const double *pc) {
  Phys f{};
  f.on = phys != nullptr;
  if (!f.on) return f;
  f.pois = phys[2] != 0.f;
  f.s = state;
  f.pc = pc;
  f.inv_dt = 1.0 / dt;
  f.inv_2dx = 1.0 / (2.0 * dx);
  f.nu_dx2 = nu / (dx * dx);
  return f;
}

// LDS: c[nx] (double) | p_n - 1, r~ (float), later q_c, q_m (double)
inline size_t lds_bytes(const Phys &f, int nx) { return f.on ? (size_t)nx * 16 : 0; }

}  // namespace

bool pinn_unroll_nx_ok(int nx) { return nx >= 1 && nx <= kFvLdsMaxNx; }

// four loss partials per IC (data, cont, mom, pois); cons: two more (energy, charge)
static LossWs carve_pinn_unroll_ws(int B, bool cons, void *base) {
  return carve_loss_ws(4 * (size_t)B, cons ? 2 * (size_t)B : 0, base);
}
int64_t pinn_unroll_ws_bytes(int B, int) { return (int64_t)carve_pinn_unroll_ws(B, false, nullptr).bytes; }
int64_t pinn_unroll_ws_bytes_ex(int B, int) { return (int64_t)carve_pinn_unroll_ws(B, true, nullptr).bytes; }

namespace {

template <bool EX>
hipError_t loss_launch(const float *pred, const float *state, const float *target, int B, int nx, const float *w,
                       float scale, const float *phys, float phys_scale, double dt, double dx, double nu,
                       const double *pc, float *losses, void *ws, const ConsTerms *cons, hipStream_t s) {
  LossArgs a{};
  a.p = pred, a.t = target;
  a.f = phys_of(state, phys, dt, dx, nu, pc);
  a.B = B, a.nx = nx;
  a.w0 = w[0], a.w1 = w[1], a.w2 = w[2];
  a.scale = (double)scale;
  if (phys) {
    a.sc = (double)phys_scale * (double)phys[0];
    a.sm = (double)phys_scale * (double)phys[1];
    a.sp = (double)phys_scale * (double)phys[2];
  }
  const LossWs lw = carve_pinn_unroll_ws(B, cons != nullptr, ws);
  a.cnt = lw.cnt;
  a.part = lw.part;
  a.losses = losses;
  if (cons) cons_setup(a.c, *cons, lw.cons_part);
  // the arrival counter starts every launch at 0 (a memset node, not a kernel)
  if (hipError_t e = hipMemsetAsync(lw.cnt, 0, 16, s)) return e;
  hipLaunchKernelGGL(pinn_unroll_loss_kernel<EX>, dim3((unsigned)B), dim3(kPuThreads), lds_bytes(a.f, nx), s, a);
  return hipGetLastError();
}

template <bool EX>
hipError_t adjoint_launch(const float *pred, const float *state, const float *target, const float *pred_next,
                          const float *grad_state_next, int B, int nx, const float *w, float scale, const float *phys,
                          float phys_scale, double dt, double dx, double nu, const double *pc, float *grad_out,
                          const float *coef, hipStream_t s) {
  AdjArgs a{};
  a.p = pred, a.t = target;
  a.f = phys_of(state, phys, dt, dx, nu, pc);
  a.pnext = phys ? pred_next : nullptr;
  a.carry = grad_state_next;
  a.nx = nx;
  a.gd0 = 2.0 * (double)w[0] * (double)scale;
  a.gd1 = 2.0 * (double)w[1] * (double)scale;
  a.gd2 = 2.0 * (double)w[2] * (double)scale;
  if (phys) {
    a.qc = 2.0 * (double)phys_scale * (double)phys[0];
    a.qm = 2.0 * (double)phys_scale * (double)phys[1];
    a.gc = a.qc / dt;
    a.gm = a.qm / dt;
    a.gp = 2.0 * (double)phys_scale * (double)phys[2];
  }
  a.g = grad_out;
  a.coef = coef;
  hipLaunchKernelGGL(pinn_unroll_adjoint_kernel<EX>, dim3((unsigned)B), dim3(kPuThreads), lds_bytes(a.f, nx), s, a);
  return hipGetLastError();
}

}  // namespace

// ex picks the instantiation; the plain entry points pass cons / coef NULL
hipError_t launch_pinn_unroll_loss(bool ex, const float *pred, const float *state, const float *target, int B, int nx,
                                   const float *w, float scale, const float *phys, float phys_scale, double dt,
                                   double dx, double nu, const double *pc, float *losses, void *ws,
                                   const ConsTerms *cons, hipStream_t s) {
  if (!pinn_unroll_nx_ok(nx) || B < 1) return hipErrorInvalidValue;
  return (ex ? loss_launch<true> : loss_launch<false>)(pred, state, target, B, nx, w, scale, phys, phys_scale, dt, dx,
                                                        nu, pc, losses, ws, ex ? cons : nullptr, s);
}

hipError_t launch_pinn_unroll_adjoint(bool ex, const float *pred, const float *state, const float *target,
                                      const float *pred_next, const float *grad_state_next, int B, int nx,
                                      const float *w, float scale, const float *phys, float phys_scale, double dt,
                                      double dx, double nu, const double *pc, float *grad_out, const float *coef,
                                      hipStream_t s) {
  if (!pinn_unroll_nx_ok(nx) || B < 1) return hipErrorInvalidValue;
  return (ex ? adjoint_launch<true> : adjoint_launch<false>)(pred, state, target, pred_next, grad_state_next, B, nx, w,
                                                              scale, phys, phys_scale, dt, dx, nu, pc, grad_out, coef,
                                                              s);
}

}  // namespace hf
