// Unrolled training: the hybrid update of one solver step with the next
// step's node features and the step's loss term (hf_unroll_update), and its
// adjoint (hf_unroll_adjoint), one launch each (src/hybrid_solver.py:45-63
// under a K-step loss; include/hybridflux.h has the mathematics).
//
// Kernel shapes follow fv_poisson.hip: FFT sizes (power-of-two nx in
// 256..2048) give one wave a pair of ICs; every other nx <= kFvLdsMaxNx gives
// one 256-thread workgroup an IC, with the circulant column and the rows in
// LDS.  The forward's arithmetic is fv_step_kernel<true>'s / fv_step_fft_kernel
// <true>'s, expression for expression (continuity, velocity_hybrid,
// poisson_cell / poisson_wave_tw of hf_device.h), so state_next equals
// launch_fv_step's bit for bit.  The adjoint applies the same operator to the
// raw gradient row (no n - 1 subtraction): P is an antisymmetric circulant
// whose rows sum to 0, so P^T e = -P e.
#include "hf_device.h"
#include "hf_internal.h"
#include "unroll_common.h"

namespace hf {
namespace {

constexpr int kUnThreads = 256;
typedef float un_f4 __attribute__((ext_vector_type(4)));

// Workspace: [0, kCounterBytes) the arrival counter, then one float64 loss
// partial per IC; the _ex calls with the conservation terms add two float64
// values per IC behind them (lam_e r_e^2, lam_q r_q^2).
struct LossArgs : StateLossArgs {};  // part [B]
struct ConsArgs : StateConsArgs {};  // part [B][2] (lam_e r_e^2, lam_q r_q^2)

// One IC's complete sums -> its two coefficients and its two term partials, by
// the one lane that holds them.
__device__ __forceinline__ void cons_finish(const ConsArgs &ca, int64_t b, int nx, double su2, double sE2, double sn) {
  cons_terms(ca, b, su2, sE2, sn, nx, ca.part[2 * b], ca.part[2 * b + 1]);
}

// The step's loss from the per-IC partials, by the wave that arrives last.
// Called by a whole wave after its partial stores; `total` waves call it per
// launch (arrival_ticket).  The partials are summed in IC order per lane and
// then across the lanes in a fixed tree, so the value does not depend on which
// wave arrives last.
template <bool EX>
__device__ __forceinline__ void loss_arrive(const LossArgs &la, const ConsArgs &ca, unsigned total, int B, int lane) {
  if (arrival_ticket(la.cnt, lane) != total - 1) return;
  acquire_partials();
  const double *part = la.part;
  double a = 0.0;
  for (int i = lane; i < B; i += 64) a += part[i];
  a = wave_sum(a);
  if constexpr (!EX) {
    if (lane == 0) la.loss[0] = (float)(a * la.scale);
  } else {
    // (total, state, energy, charge): the state value is the plain call's
    double e = 0.0, q = 0.0;
    if (ca.on) {
      for (int i = lane; i < B; i += 64) e += ca.part[2 * i], q += ca.part[2 * i + 1];
      e = wave_sum(e);
      q = wave_sum(q);
    }
    if (lane == 0) {
      const double ls = a * la.scale, le = e * ca.scale, lq = q * ca.scale;
      la.loss[0] = ca.on ? (float)((ls + le) + lq) : (float)ls;
      la.loss[1] = (float)ls;
      la.loss[2] = (float)le;
      la.loss[3] = (float)lq;
    }
  }
}

// ------------------------------------------------------- forward, circulant nx
// LDS: red[4] | c[nx] (double) | u, F, rho (float)
inline size_t update_lds_bytes(int nx) { return 4 * sizeof(double) + (size_t)nx * (sizeof(double) + 3 * sizeof(float)); }

template <bool EX>
__global__ __launch_bounds__(kUnThreads) void unroll_update_kernel(const float *__restrict__ fe,
                                                                   const float *__restrict__ in,
                                                                   const float *__restrict__ x,
                                                                   const double *__restrict__ pc, int nx, float c,
                                                                   float dt, float *out, float *nf, LossArgs la, int B,
                                                                   ConsArgs ca) {
  extern __shared__ double s_dyn[];
  double *red = s_dyn, *Lc = s_dyn + 4;
  float *Lu = reinterpret_cast<float *>(Lc + nx), *LF = Lu + nx, *Lrho = LF + nx;
  const int64_t b = blockIdx.x;
  const float *st = in + b * 3 * nx, *feb = fe + b * 2 * nx;
  float *so = out + b * 3 * nx;
  for (int i = threadIdx.x; i < nx; i += kUnThreads) {
    Lu[i] = st[nx + i];
    LF[i] = face_flux(feb[i], feb[nx + i]);
    Lc[i] = pc[i];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nx; i += kUnThreads) {
    const int im = i == 0 ? nx - 1 : i - 1;
    const float n_new = continuity(st[i], LF[i], LF[im], c);
    const float u_new = velocity_hybrid(Lu[i], Lu[im], st[2 * nx + i], c, dt);
    Lrho[i] = __fsub_rn(n_new, 1.0f);
    so[i] = n_new;
    so[nx + i] = u_new;
  }
  __syncthreads();
  const float *tg = la.tgt ? la.tgt + b * 3 * nx : nullptr;
  const bool cons = EX && ca.on;
  double acc = 0.0, su2 = 0.0, sE2 = 0.0, sn = 0.0;
  for (int i = threadIdx.x; i < nx; i += kUnThreads) {
    const float E_new = poisson_cell(Lrho, Lc, i, nx);
    so[2 * nx + i] = E_new;
    const float n_new = so[i], u_new = so[nx + i];  // this thread's own stores
    if (nf) *reinterpret_cast<un_f4 *>(nf + 4 * (b * nx + i)) = un_f4{n_new, u_new, E_new, x[i]};
    if (tg) acc += sq_err(n_new, tg[i], la.w0) + sq_err(u_new, tg[nx + i], la.w1) + sq_err(E_new, tg[2 * nx + i], la.w2);
    if (cons) {
      su2 += (double)u_new * (double)u_new;
      sE2 += (double)E_new * (double)E_new;
      sn += (double)n_new;
    }
  }
  if (!tg) return;  // (uniform)
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  if constexpr (EX) {
    __shared__ double redc[3][4];
    if (cons) {  // (uniform)
      su2 = wave_sum(su2);
      sE2 = wave_sum(sE2);
      sn = wave_sum(sn);
      if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        redc[0][wv] = su2, redc[1][wv] = sE2, redc[2][wv] = sn;
      }
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    if (threadIdx.x == 0) {
      la.part[b] = ((red[0] + red[1]) + red[2]) + red[3];
      if (cons)
        cons_finish(ca, b, nx, ((redc[0][0] + redc[0][1]) + redc[0][2]) + redc[0][3],
                    ((redc[1][0] + redc[1][1]) + redc[1][2]) + redc[1][3],
                    ((redc[2][0] + redc[2][1]) + redc[2][2]) + redc[2][3]);
    }
  } else {
    __syncthreads();
    if (threadIdx.x >= 64) return;
    if (threadIdx.x == 0) la.part[b] = ((red[0] + red[1]) + red[2]) + red[3];
  }
  loss_arrive<EX>(la, ca, gridDim.x, B, threadIdx.x);
}

// ------------------------------------------------------------ forward, FFT sizes
// One IC's update on the wave's registers (fv_update_in<true, N>'s expressions).
template <int N>
__device__ __forceinline__ void update_ic(const float *__restrict__ st, const float *__restrict__ feb, float *so, float c,
                                          float dt, int lane, double (&rho)[N / 64]) {
  constexpr int V = N / 64;
  float n[V], u[V], E[V], F[V], ul[V], Fl[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int cell = lane + 64 * i;
    n[i] = st[cell];
    u[i] = st[N + cell];
    E[i] = st[2 * N + cell];
    F[i] = face_flux(feb[cell], feb[N + cell]);
  }
  left_of<V>(u, ul);
  left_of<V>(F, Fl);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int cell = lane + 64 * i;
    const float n_new = continuity(n[i], F[i], Fl[i], c);
    so[cell] = n_new;
    so[N + cell] = velocity_hybrid(u[i], ul[i], E[i], c, dt);
    rho[i] = (double)__fsub_rn(n_new, 1.0f);
  }
}

// E' of one IC of the pair, the next node features and the IC's loss partial.
template <int N, bool IMAG, bool EX>
__device__ __forceinline__ void finish_ic(float *so, const double2 (&v)[N / 64], const float *__restrict__ x, float *nfb,
                                          const float *tg, const LossArgs &la, const ConsArgs &ca, int64_t ic, int lane) {
  const bool cons = EX && ca.on && tg;
  double acc = 0.0, su2 = 0.0, sE2 = 0.0, sn = 0.0;
#pragma unroll
  for (int i = 0; i < N / 64; ++i) {
    const int cell = lane + 64 * i;
    const float E_new = (float)((IMAG ? v[i].y : v[i].x) / N);
    so[2 * N + cell] = E_new;
    const float n_new = so[cell], u_new = so[N + cell];  // this lane's own stores
    if (nfb) *reinterpret_cast<un_f4 *>(nfb + 4 * cell) = un_f4{n_new, u_new, E_new, x[cell]};
    if (tg) acc += sq_err(n_new, tg[cell], la.w0) + sq_err(u_new, tg[N + cell], la.w1) + sq_err(E_new, tg[2 * N + cell], la.w2);
    if (cons) {
      su2 += (double)u_new * (double)u_new;
      sE2 += (double)E_new * (double)E_new;
      sn += (double)n_new;
    }
  }
  if (tg) {
    acc = wave_sum(acc);
    if (lane == 0) la.part[ic] = acc;
  }
  if (cons) {
    su2 = wave_sum(su2);
    sE2 = wave_sum(sE2);
    sn = wave_sum(sn);
    if (lane == 0) cons_finish(ca, ic, N, su2, sE2, sn);
  }
}

template <int N, bool EX>
__global__ __launch_bounds__(64 * kFftWaves, N >= 2048 ? 1 : 2) void unroll_update_fft_kernel(
    const float *__restrict__ fe, const float *__restrict__ in, const float *__restrict__ x,
    const double *__restrict__ pc, float c, float dt, float *out, float *nf, LossArgs la, int B, ConsArgs ca) {
  constexpr int V = N / 64;
  __shared__ double2 s_fft[kFftWaves][fft_lds_elems<N>()];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t a = 2 * ((int64_t)blockIdx.x * kFftWaves + wave), b = a + 1;
  if (a >= B) return;  // a whole wave; nothing below synchronises the workgroup
  const bool two = b < B;
  double *rho_a = reinterpret_cast<double *>(s_fft[wave]);  // the transform's buffer, free until it starts
  double2 v[V];
  {
    double r[V];
    update_ic<N>(in + a * 3 * N, fe + a * 2 * N, out + a * 3 * N, c, dt, lane, r);
#pragma unroll
    for (int i = 0; i < V; ++i) rho_a[lane + 64 * i] = r[i];  // parked while IC b's update holds the registers
  }
  {
    double r[V];
    if (two) update_ic<N>(in + b * 3 * N, fe + b * 2 * N, out + b * 3 * N, c, dt, lane, r);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = make_double2(rho_a[lane + 64 * i], two ? r[i] : 0.0);
  }
  poisson_wave_tw<N>(v, s_fft[wave], reinterpret_cast<const double2 *>(pc + N), pc + 2 * N, lane);
  finish_ic<N, false, EX>(out + a * 3 * N, v, x, nf ? nf + a * 4 * N : nullptr, la.tgt ? la.tgt + a * 3 * N : nullptr,
                          la, ca, a, lane);
  if (two)
    finish_ic<N, true, EX>(out + b * 3 * N, v, x, nf ? nf + b * 4 * N : nullptr, la.tgt ? la.tgt + b * 3 * N : nullptr,
                           la, ca, b, lane);
  if (la.tgt) loss_arrive<EX>(la, ca, (unsigned)((B + 1) / 2), B, lane);
}

// --------------------------------------------------------------------- adjoint
// The total gradient dL/d s^_{k+1} of one value (channel ch, cell i of IC b):
// the previous adjoint call's direct part + the FluxGNN backward's
// d node_features (both optional) + the loss seed gs_ch (s^ - s*).  EX with
// coef [B][2] = (ce, cq): the seed of u and of E gains ce_b u, ce_b E (one
// float32 product, added to the seed before the other parts); cq_b is not
// added, the charge term has no gradient through the conservative update.
struct AdjIn {
  const float *sn, *tg;  // s^_{k+1}, s*_{k+1}  [B][3][nx]
  const float *din;      // direct part of step k+1 [B][3][nx] or NULL
  const float *gnf;      // d node_features of step k+1 [B*nx][4] or NULL
  float gs[3];           // 2 w_ch scale
  const float *coef;     // [B][2] or NULL (read by the EX kernels only)
};
template <bool EX>
__device__ __forceinline__ float total_g(const AdjIn &g, int64_t b, int ch, int i, int nx) {
  const int64_t o = b * 3 * nx + (int64_t)ch * nx + i;
  float v = g.gs[ch] * (g.sn[o] - g.tg[o]);
  if constexpr (EX) {
    if (g.coef && ch != 0) v = v + g.coef[2 * b] * g.sn[o];
  }
  if (g.gnf) v += g.gnf[4 * (b * nx + i) + ch];
  if (g.din) v += g.din[o];
  return v;
}

// LDS: c[nx] (double) | e, a~, b (float)
inline size_t adjoint_lds_bytes(int nx) { return (size_t)nx * (sizeof(double) + 3 * sizeof(float)); }

template <bool EX>
__global__ __launch_bounds__(kUnThreads) void unroll_adjoint_kernel(const float *__restrict__ st, AdjIn g,
                                                                    const double *__restrict__ pc, int nx, float c,
                                                                    float dt, float *__restrict__ g_fe,
                                                                    float *__restrict__ dout) {
  extern __shared__ double s_dyn[];
  double *Lc = s_dyn;
  float *Le = reinterpret_cast<float *>(Lc + nx), *La = Le + nx, *Lb = La + nx;
  const int64_t b = blockIdx.x;
  for (int i = threadIdx.x; i < nx; i += kUnThreads) {
    Lc[i] = pc[i];
    La[i] = total_g<EX>(g, b, 0, i, nx);
    Lb[i] = total_g<EX>(g, b, 1, i, nx);
    Le[i] = total_g<EX>(g, b, 2, i, nx);
  }
  __syncthreads();
  // a~ = a + P^T e = a - P e (only this thread reads La[i] before the barrier)
  for (int i = threadIdx.x; i < nx; i += kUnThreads) La[i] = La[i] - poisson_cell(Le, Lc, i, nx);
  __syncthreads();
  const float *u = st + b * 3 * nx + nx;
  for (int i = threadIdx.x; i < nx; i += kUnThreads) {
    const int ip = i == nx - 1 ? 0 : i + 1;
    const float at = La[i], bi = Lb[i];
    const float h = 0.5f * (-c * (at - La[ip]));  // 0.5 dL/dF_i
    g_fe[b * 2 * nx + i] = h;
    g_fe[b * 2 * nx + nx + i] = h;
    if (dout) {
      float *d = dout + b * 3 * nx;
      d[i] = at;
      d[nx + i] = bi - c * u[i] * (bi - Lb[ip]);
      d[2 * nx + i] = dt * bi;
    }
  }
}

template <int N, bool IMAG, bool EX>
__device__ __forceinline__ void adjoint_ic(const float *__restrict__ st, const AdjIn &g, const double2 (&v)[N / 64],
                                           int64_t ic, float c, float dt, float *__restrict__ g_fe,
                                           float *__restrict__ dout, int lane) {
  constexpr int V = N / 64;
  float at[V], bb[V], atr[V], bbr[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int cell = lane + 64 * i;
    at[i] = total_g<EX>(g, ic, 0, cell, N) - (float)((IMAG ? v[i].y : v[i].x) / N);
    bb[i] = total_g<EX>(g, ic, 1, cell, N);
  }
  right_of<V>(at, atr);
  right_of<V>(bb, bbr);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int cell = lane + 64 * i;
    const float h = 0.5f * (-c * (at[i] - atr[i]));
    g_fe[ic * 2 * N + cell] = h;
    g_fe[ic * 2 * N + N + cell] = h;
    if (dout) {
      float *d = dout + ic * 3 * N;
      d[cell] = at[i];
      d[N + cell] = bb[i] - c * st[ic * 3 * N + N + cell] * (bb[i] - bbr[i]);
      d[2 * N + cell] = dt * bb[i];
    }
  }
}

template <int N, bool EX>
__global__ __launch_bounds__(64 * kFftWaves, N >= 2048 ? 1 : 2) void unroll_adjoint_fft_kernel(
    const float *__restrict__ st, AdjIn g, const double *__restrict__ pc, float c, float dt, float *__restrict__ g_fe,
    float *__restrict__ dout, int B) {
  constexpr int V = N / 64;
  __shared__ double2 s_fft[kFftWaves][fft_lds_elems<N>()];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t a = 2 * ((int64_t)blockIdx.x * kFftWaves + wave), b = a + 1;
  if (a >= B) return;  // a whole wave; nothing below synchronises the workgroup
  const bool two = b < B;
  double2 v[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int cell = lane + 64 * i;
    v[i] = make_double2((double)total_g<EX>(g, a, 2, cell, N), two ? (double)total_g<EX>(g, b, 2, cell, N) : 0.0);
  }
  poisson_wave_tw<N>(v, s_fft[wave], reinterpret_cast<const double2 *>(pc + N), pc + 2 * N, lane);  // N P e
  adjoint_ic<N, false, EX>(st, g, v, a, c, dt, g_fe, dout, lane);
  if (two) adjoint_ic<N, true, EX>(st, g, v, b, c, dt, g_fe, dout, lane);
}

// ex: the _ex entry points' instantiation (the wider loss row, the conservation terms, the coefficients)
template <int N>
hipError_t update_fft_launch(const float *fe, const float *st, const float *x, const double *pc, int B, float c, float dt,
                             float *out, float *nf, const LossArgs &la, const ConsArgs &ca, bool ex, hipStream_t s) {
  const unsigned grid = (unsigned)((B + 2 * kFftWaves - 1) / (2 * kFftWaves));
  if (ex)
    hipLaunchKernelGGL((unroll_update_fft_kernel<N, true>), dim3(grid), dim3(64 * kFftWaves), 0, s, fe, st, x, pc, c, dt,
                       out, nf, la, B, ca);
  else
    hipLaunchKernelGGL((unroll_update_fft_kernel<N, false>), dim3(grid), dim3(64 * kFftWaves), 0, s, fe, st, x, pc, c, dt,
                       out, nf, la, B, ca);
  return hipGetLastError();
}
template <int N>
hipError_t adjoint_fft_launch(const float *st, const AdjIn &g, const double *pc, int B, float c, float dt, float *g_fe,
                              float *dout, bool ex, hipStream_t s) {
  const unsigned grid = (unsigned)((B + 2 * kFftWaves - 1) / (2 * kFftWaves));
  if (ex)
    hipLaunchKernelGGL((unroll_adjoint_fft_kernel<N, true>), dim3(grid), dim3(64 * kFftWaves), 0, s, st, g, pc, c, dt,
                       g_fe, dout, B);
  else
    hipLaunchKernelGGL((unroll_adjoint_fft_kernel<N, false>), dim3(grid), dim3(64 * kFftWaves), 0, s, st, g, pc, c, dt,
                       g_fe, dout, B);
  return hipGetLastError();
}

}  // namespace

bool unroll_nx_ok(int nx) { return nx >= 1 && nx <= kFvLdsMaxNx; }

// one loss partial per IC; cons: two more (energy, charge)
static LossWs carve_unroll_ws(int B, bool cons, void *base) { return carve_loss_ws((size_t)B, cons ? 2 * (size_t)B : 0, base); }
int64_t unroll_ws_bytes(int B, int) { return (int64_t)carve_unroll_ws(B, false, nullptr).bytes; }
int64_t unroll_ws_bytes_ex(int B, int) { return (int64_t)carve_unroll_ws(B, true, nullptr).bytes; }

hipError_t launch_unroll_update(bool ex, const float *fe, const float *st, const float *x, const double *pc, int B,
                                int nx, float c, float dt, float *st_next, float *nf_next, const float *target,
                                const float *w, float scale, float *loss, void *ws, const ConsTerms *cons,
                                hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (!unroll_nx_ok(nx)) return hipErrorInvalidValue;
  LossArgs la{};
  ConsArgs ca{};
  if (target) {
    if (!ex) cons = nullptr;
    const hipError_t e = state_loss_setup(la, ca, target, w, scale, loss, carve_unroll_ws(B, cons != nullptr, ws), cons, s);
    if (e) return e;
  }
  switch (poisson_uses_fft(nx) ? nx : 0) {
    case 256: return update_fft_launch<256>(fe, st, x, pc, B, c, dt, st_next, nf_next, la, ca, ex, s);
    case 512: return update_fft_launch<512>(fe, st, x, pc, B, c, dt, st_next, nf_next, la, ca, ex, s);
    case 1024: return update_fft_launch<1024>(fe, st, x, pc, B, c, dt, st_next, nf_next, la, ca, ex, s);
    case 2048: return update_fft_launch<2048>(fe, st, x, pc, B, c, dt, st_next, nf_next, la, ca, ex, s);
    default: break;
  }
  if (ex)
    hipLaunchKernelGGL(unroll_update_kernel<true>, dim3((unsigned)B), dim3(kUnThreads), update_lds_bytes(nx), s, fe, st, x,
                       pc, nx, c, dt, st_next, nf_next, la, B, ca);
  else
    hipLaunchKernelGGL(unroll_update_kernel<false>, dim3((unsigned)B), dim3(kUnThreads), update_lds_bytes(nx), s, fe, st, x,
                       pc, nx, c, dt, st_next, nf_next, la, B, ca);
  return hipGetLastError();
}

hipError_t launch_unroll_adjoint(bool ex, const float *st, const float *st_next, const float *target, const float *w,
                                 float scale, const float *direct_next, const float *gnf_next, const double *pc, int B,
                                 int nx, float c, float dt, float *g_fe, float *direct, const float *coef,
                                 hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (!unroll_nx_ok(nx)) return hipErrorInvalidValue;
  AdjIn g{};
  g.sn = st_next;
  g.tg = target;
  g.din = direct_next;
  g.gnf = gnf_next;
  g.coef = coef;
  for (int k = 0; k < 3; ++k) g.gs[k] = (float)(2.0 * (double)w[k] * (double)scale);
  switch (poisson_uses_fft(nx) ? nx : 0) {
    case 256: return adjoint_fft_launch<256>(st, g, pc, B, c, dt, g_fe, direct, ex, s);
    case 512: return adjoint_fft_launch<512>(st, g, pc, B, c, dt, g_fe, direct, ex, s);
    case 1024: return adjoint_fft_launch<1024>(st, g, pc, B, c, dt, g_fe, direct, ex, s);
    case 2048: return adjoint_fft_launch<2048>(st, g, pc, B, c, dt, g_fe, direct, ex, s);
    default: break;
  }
  if (ex)
    hipLaunchKernelGGL(unroll_adjoint_kernel<true>, dim3((unsigned)B), dim3(kUnThreads), adjoint_lds_bytes(nx), s, st, g,
                       pc, nx, c, dt, g_fe, direct);
  else
    hipLaunchKernelGGL(unroll_adjoint_kernel<false>, dim3((unsigned)B), dim3(kUnThreads), adjoint_lds_bytes(nx), s, st, g,
                       pc, nx, c, dt, g_fe, direct);
  return hipGetLastError();
}

}  // namespace hf
