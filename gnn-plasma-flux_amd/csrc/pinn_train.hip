// PINN training (scripts/training/train_pinn.py:48-61 under loss.backward(),
// :64-111, :156-179): the forward that keeps an activation tape, the backward,
// and the physics loss of :163-175 with its gradient in one launch.
//
// Network: layer 0 D->H tanh, layers 1..L-2 H->H tanh, layer L-1 H->D, out =
// state + net(state); parameters flat in state-dict order (weight, bias per
// layer).  Tape: the L-1 tanh activations a_0..a_{L-2}, [B][H] each, 256-byte
// aligned, in this order.
//
// Backward, given g = dL/dout [B][D] (G_{L-1} = g):
//   layer l   gW_l = G_l^T a_{l-1} (a_{-1} = state), gb_l = column sums of G_l,
//             G_{l-1} = (G_l W_l) * (1 - a_{l-1}^2)
//   state     dL/dstate = g + G_0 W_0 (on request)
// Two paths:
//   GEMM     D % 32 == 0 and H % 32 == 0 (the reference's PINN(192, 256)):
//            tgemm.h f32 MFMA GEMMs.  Forward: EpiTanh, and EpiBiasResid for
//            the last layer; data gradients: EpiTanhGrad; weight gradients:
//            split-K EpiPart partials with COLSUM for the bias (the L-2 hidden
//            layers, one shape, as ONE tgemm_batch launch), and one
//            fixed-order reduction of every layer's partials.  L forward
//            launches, L + 3 backward ones (+ 1 with dL/dstate; L = 2: L + 2).
//   generic  every other shape: gemm_linear / gemm_wgrad of graph.hip.
// Every sum has a fixed order: two calls give the same bits.
//
// Loss (pinn_loss_kernel): one 256-thread workgroup per IC; the circulant
// column of the spectral Poisson operator P (double), p_n - 1 and r~ in LDS;
// P (p_n - 1) and P r~ by poisson_cell (hf_device.h), the solver's own sum.
// Residuals and sums in float64; per-IC partials, summed by the last workgroup
// to arrive in a fixed order.  No float atomics.
#include <algorithm>

#include "hf_device.h"
#include "hf_internal.h"
#include "tgemm.h"
#include "unroll_common.h"

namespace hf {
namespace {

using namespace tg;

struct PinnV {
  const float *w[kMaxChainLayers], *b[kMaxChainLayers];
  int in[kMaxChainLayers], out[kMaxChainLayers];
};
PinnV pinn_train_view(const float *p, int D, int H, int L) {
  PinnV v{};
  int64_t o = 0;
  for (int l = 0; l < L; ++l) {
    v.in[l] = l == 0 ? D : H;
    v.out[l] = l == L - 1 ? D : H;
    v.w[l] = p + o;
    o += (int64_t)v.in[l] * v.out[l];
    v.b[l] = p + o;
    o += v.out[l];
  }
  return v;
}

inline bool pinn_gemm_path(int D, int H, int64_t B) {
  return D % 32 == 0 && H % 32 == 0 && (B + 1) * std::max(D, H) < (int64_t(1) << 31);
}

// weight-gradient splits of the GEMM path: 128 batch rows each, at most 64
inline int pinn_wg_splits(int64_t B) { return (int)std::min<int64_t>(64, std::max<int64_t>(1, (B + 127) / 128)); }

struct PinnTape {
  float *a[kMaxChainLayers];
  size_t bytes;
};
PinnTape carve_pinn_tape(int H, int L, int64_t B, void *base) {
  Carve c(base);
  PinnTape t{};
  for (int l = 0; l + 1 < L; ++l) t.a[l] = c.take<float>(B * H);
  t.bytes = c.off;
  return t;
}

struct PinnBws {
  float *g[kMaxChainLayers];                             // G_0..G_{L-2}, [B][H] each
  float *part[kMaxChainLayers], *bpart[kMaxChainLayers];  // GEMM path: [S][out][in], [S][out] per layer
  float *gpart;                                          // generic path: gemm_wgrad's partials
  size_t bytes;
};
PinnBws carve_pinn_bws(int D, int H, int L, int64_t B, void *base) {
  Carve c(base);
  PinnBws w{};
  for (int l = 0; l + 1 < L; ++l) w.g[l] = c.take<float>(B * H);
  if (pinn_gemm_path(D, H, B)) {
    const int64_t S = tgemm_splits(B, pinn_wg_splits(B));
    for (int l = 0; l < L; ++l) {
      const int64_t in = l == 0 ? D : H, out = l == L - 1 ? D : H;
      w.part[l] = c.take<float>(S * out * in);
      w.bpart[l] = c.take<float>(S * out);
    }
  } else {
    w.gpart = c.take<float>(std::max(gemm_wgrad_part_floats(B, H, D),
                                     std::max(gemm_wgrad_part_floats(B, H, H), gemm_wgrad_part_floats(B, D, H))));
  }
  w.bytes = c.off;
  return w;
}

__device__ __forceinline__ float tanh_bwd(float g, float y) { return __fmul_rn(g, __fsub_rn(1.f, __fmul_rn(y, y))); }

// out[i][j] = resid[i][j] + (v + bias[j]): the last layer with the residual state (train_pinn.py:61)
struct EpiBiasResid {
  float *out;
  int64_t ld;
  const float *bias, *resid;
  __device__ float bias_of(int64_t j) const { return bias[j]; }
  static constexpr bool kPre = false, kBlock = false;
  __device__ float pre(int64_t, int64_t) const { return 0.f; }
  __device__ void operator()(int64_t i, int64_t j, float v, float bj, float) const {
    out[i * ld + j] = __fadd_rn(resid[i * ld + j], __fadd_rn(v, bj));
  }
};

// Data-gradient epilogue: out = (resid + v) * (1 - y^2), y the layer's tanh
// output on the tape; resid and y optional (neither may alias out).
struct EpiTanhGrad {
  float *out;
  int64_t ld;
  const float *resid, *y;
  __device__ float bias_of(int64_t) const { return 0.f; }
  static constexpr bool kPre = false, kBlock = false;
  __device__ float pre(int64_t, int64_t) const { return 0.f; }
  __device__ void operator()(int64_t i, int64_t j, float v, float, float) const {
    if (resid) v = __fadd_rn(resid[i * ld + j], v);
    if (y) v = tanh_bwd(v, y[i * ld + j]);
    out[i * ld + j] = v;
  }
};

// out = g * (1 - y^2) (generic path; out may be g)
__global__ void pinn_tanh_grad_kernel(const float *g, const float *__restrict__ y, int64_t n, float *out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = tanh_bwd(g[t], y[t]);
}

// The fixed-order reduction of every layer's split-K partials (EpiPart's
// [S][I][J], COLSUM's [S][I]) in one launch: grid y = layer, splits ascending.
struct PinnRed {
  const float *part[kMaxChainLayers], *bpart[kMaxChainLayers];
  float *gw[kMaxChainLayers], *gb[kMaxChainLayers];
  int I[kMaxChainLayers], J[kMaxChainLayers];
};
__global__ __launch_bounds__(256) void pinn_part_reduce_kernel(PinnRed r, int S) {
  const int l = blockIdx.y;
  const int I = r.I[l];
  const int64_t n = (int64_t)I * r.J[l], t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n + I) return;
  const bool is_w = t < n;
  const float *src = is_w ? r.part[l] + t : r.bpart[l] + (t - n);
  const int64_t st = is_w ? n : I;
  float v = 0.f;
  for (int s = 0; s < S; ++s) v = __fadd_rn(v, src[(int64_t)s * st]);
  if (is_w) r.gw[l][t] = v;
  else r.gb[l][t - n] = v;
}

inline VPlain mat(const float *p, int64_t rows, int cols) { return VPlain{p, cols, rows, kNoSplit, 0, cols}; }

// ------------------------------------------------------------------- the loss
constexpr int kLossThreads = 256;
// Workspace (unroll_common.h LossWs): the arrival counter, then four float64
// partials per IC (data, cont, mom, pois).
LossWs carve_pinn_loss_ws(int B, void *base) { return carve_loss_ws(4 * (size_t)B, 0, base); }

struct PinnLossArgs {
  const float *p, *s, *sn;  // pred, state_t, state_next [B][3][nx]
  const double *pc;         // the circulant column, plan[0..nx)
  int B, nx;
  double inv_dt, inv_2dx, nu_dx2;
  double gd, gc, gm, gp;    // 2 w_d / N3, 2 w_c / (dt N1), 2 w_m / (dt N1), 2 w_p / N1
  double inv_n3, inv_n1;
  double w[4];
  double *part;             // [B][4]
  unsigned *cnt;
  float *losses, *g;
};

// LDS: c[nx] (double) | p_n - 1, r~ (float)
inline size_t pinn_loss_lds_bytes(int nx) { return (size_t)nx * (sizeof(double) + 2 * sizeof(float)); }

__global__ __launch_bounds__(kLossThreads) void pinn_loss_kernel(PinnLossArgs a) {
  extern __shared__ double s_dyn[];
  __shared__ double red[4][4];
  const int nx = a.nx;
  double *Lc = s_dyn;
  float *Lrho = reinterpret_cast<float *>(Lc + nx), *Lrt = Lrho + nx;
  const int64_t b = blockIdx.x;
  const float *P = a.p + b * 3 * nx, *S = a.s + b * 3 * nx, *T = a.sn + b * 3 * nx;
  float *G = a.g + b * 3 * nx;
  for (int i = threadIdx.x; i < nx; i += kLossThreads) {
    Lc[i] = a.pc[i];
    Lrho[i] = __fsub_rn(P[i], 1.0f);  // P has zero row sums: P p_n = P (p_n - 1), the solver's operand
  }
  __syncthreads();
  double sd = 0.0, sc = 0.0, sm = 0.0, sp = 0.0;
  for (int i = threadIdx.x; i < nx; i += kLossThreads) {
    const int ip = i == nx - 1 ? 0 : i + 1, im = i == 0 ? nx - 1 : i - 1;
    const double n = S[i], u = S[nx + i], E = S[2 * nx + i];
    const double up = S[nx + ip], um = S[nx + im];
    const double pn = P[i], pu = P[nx + i], pE = P[2 * nx + i];
    const double dn = pn - (double)T[i], du = pu - (double)T[nx + i], dE = pE - (double)T[2 * nx + i];
    const double rc = (pn - n) * a.inv_dt + ((double)S[ip] * up - (double)S[im] * um) * a.inv_2dx;
    const double rm = (pu - u) * a.inv_dt + u * (up - um) * a.inv_2dx + E - a.nu_dx2 * (up - 2.0 * u + um);
    // X[0] = 0, X[i] = -(P p_n)[i]; r~ = r_p with cell 0 zeroed (train_pinn.py:72-74)
    const double X = i == 0 ? 0.0 : -(double)poisson_cell(Lrho, Lc, i, nx);
    const double rp = pE - X;
    Lrt[i] = i == 0 ? 0.f : (float)rp;
    sd += dn * dn + du * du + dE * dE;
    sc += rc * rc;
    sm += rm * rm;
    sp += rp * rp;
    G[i] = (float)(a.gd * dn + a.gc * rc);  // the P r~ term is added below
    G[nx + i] = (float)(a.gd * du + a.gm * rm);
    G[2 * nx + i] = (float)(a.gd * dE + a.gp * rp);
  }
  __syncthreads();
  // dL/dp_n -= (2 w_p / N1) (P r~)   (P^T = -P; this thread's own store above)
  for (int i = threadIdx.x; i < nx; i += kLossThreads)
    G[i] = (float)((double)G[i] - a.gp * (double)poisson_cell(Lrt, Lc, i, nx));
  sd = wave_sum(sd);
  sc = wave_sum(sc);
  sm = wave_sum(sm);
  sp = wave_sum(sp);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave][0] = sd, red[wave][1] = sc, red[wave][2] = sm, red[wave][3] = sp;
  __syncthreads();
  if (threadIdx.x >= 64) return;
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
  if (lane == 0) {
    const double ld = q[0] * a.inv_n3, lc = q[1] * a.inv_n1, lm = q[2] * a.inv_n1, lp = q[3] * a.inv_n1;
    a.losses[0] = (float)(a.w[0] * ld + a.w[1] * lc + a.w[2] * lm + a.w[3] * lp);
    a.losses[1] = (float)ld;
    a.losses[2] = (float)lc;
    a.losses[3] = (float)lm;
    a.losses[4] = (float)lp;
  }
}

}  // namespace

int64_t pinn_tape_bytes(int H, int L, int64_t B) { return (int64_t)carve_pinn_tape(H, L, B, nullptr).bytes; }

int64_t pinn_backward_ws_bytes(int D, int H, int L, int64_t B) {
  return (int64_t)carve_pinn_bws(D, H, L, B, nullptr).bytes;
}

hipError_t launch_pinn_forward_train(const float *params, int D, int H, int L, const float *state, int64_t B, float *out,
                                     void *tape, hipStream_t s) {
  const PinnV w = pinn_train_view(params, D, H, L);
  const PinnTape t = carve_pinn_tape(H, L, B, tape);
  const bool gemm = pinn_gemm_path(D, H, B);
  hipError_t e;
  const float *in = state;
  for (int l = 0; l + 1 < L; ++l) {
    if (gemm)
      e = tgemm<VPlain, false, VPlain, false, EpiTanh>(mat(in, B, w.in[l]), mat(w.w[l], H, w.in[l]),
                                                       EpiTanh{t.a[l], H, w.b[l]}, B, H, w.in[l], 1, s);
    else
      e = gemm_linear(in, w.in[l], nullptr, nullptr, 0, nullptr, wv_rows(w.w[l], w.in[l], w.in[l]), w.b[l], t.a[l], B, H,
                      kActTanh, nullptr, s);
    if (e) return e;
    in = t.a[l];
  }
  if (gemm)
    return tgemm<VPlain, false, VPlain, false, EpiBiasResid>(mat(in, B, H), mat(w.w[L - 1], D, H),
                                                             EpiBiasResid{out, D, w.b[L - 1], state}, B, D, H, 1, s);
  return gemm_linear(in, H, nullptr, nullptr, 0, nullptr, wv_rows(w.w[L - 1], H, H), w.b[L - 1], out, B, D, kActNone,
                     state, s);
}

hipError_t launch_pinn_backward(const float *params, int D, int H, int L, const float *state, int64_t B,
                                const void *tape, const float *grad_out, float *grad_params, float *grad_state,
                                void *ws, hipStream_t s) {
  const PinnV w = pinn_train_view(params, D, H, L);
  const PinnV gv = pinn_train_view(grad_params, D, H, L);
  auto mut = [](const float *p) { return const_cast<float *>(p); };
  const PinnTape t = carve_pinn_tape(H, L, B, const_cast<void *>(tape));
  const PinnBws b = carve_pinn_bws(D, H, L, B, ws);
  // G_l = dL/d(pre-activation of layer l) and X_l = the layer's input
  auto G = [&](int l) { return l == L - 1 ? grad_out : b.g[l]; };
  auto X = [&](int l) { return l == 0 ? state : t.a[l - 1]; };
  hipError_t e;
  if (pinn_gemm_path(D, H, B)) {
    // data gradients, last layer first: G_{l-1} = (G_l W_l) * (1 - a_{l-1}^2)
    for (int l = L - 1; l >= 1; --l)
      if ((e = tgemm<VPlain, false, VPlain, true, EpiTanhGrad>(mat(G(l), B, w.out[l]), mat(w.w[l], w.out[l], H),
                                                               EpiTanhGrad{b.g[l - 1], H, nullptr, t.a[l - 1]}, B, H,
                                                               w.out[l], 1, s)))
        return e;
    if (grad_state &&
        (e = tgemm<VPlain, false, VPlain, true, EpiTanhGrad>(mat(b.g[0], B, H), mat(w.w[0], H, D),
                                                             EpiTanhGrad{grad_state, D, grad_out, nullptr}, B, D, H, 1,
                                                             s)))
      return e;
    // weight gradients: gW_l = G_l^T X_l as split-K partials, gb_l from the column sums
    const int splits = pinn_wg_splits(B);
    const int S = (int)tgemm_splits(B, splits);
    for (int l : {L - 1, 0})
      if ((e = tgemm<VPlain, true, VPlain, true, EpiPart, true, true>(
               mat(G(l), B, w.out[l]), mat(X(l), B, w.in[l]), EpiPart{b.part[l], w.out[l], w.in[l]}, w.out[l], w.in[l],
               B, splits, s, b.bpart[l])))
        return e;
    if (L > 2) {  // the hidden layers' H x H problems in one launch
      TgBatch<VPlain, VPlain, EpiPart> bt{};
      bt.n = L - 2;
      for (int l = 1; l + 1 < L; ++l) {
        bt.a[l - 1] = mat(G(l), B, H);
        bt.b[l - 1] = mat(X(l), B, H);
        bt.e[l - 1] = EpiPart{b.part[l], H, H};
        bt.bias_part[l - 1] = b.bpart[l];
      }
      if ((e = tgemm_batch<VPlain, VPlain, EpiPart, true>(bt, H, H, B, splits, s))) return e;
    }
    PinnRed r{};
    int64_t nmax = 0;
    for (int l = 0; l < L; ++l) {
      r.part[l] = b.part[l], r.bpart[l] = b.bpart[l];
      r.gw[l] = mut(gv.w[l]), r.gb[l] = mut(gv.b[l]);
      r.I[l] = w.out[l], r.J[l] = w.in[l];
      nmax = std::max(nmax, (int64_t)w.out[l] * w.in[l] + w.out[l]);
    }
    hipLaunchKernelGGL(pinn_part_reduce_kernel, dim3(blocks_of(nmax), (unsigned)L), dim3(256), 0, s, r, S);
    return hipGetLastError();
  }
  for (int l = L - 1; l >= 0; --l) {
    if ((e = gemm_wgrad(G(l), w.out[l], X(l), w.in[l], B, mut(gv.w[l]), w.in[l], mut(gv.b[l]), b.gpart, s))) return e;
    if (l == 0) break;
    // G_l W_l into the tape-sized scratch of G_{l-1}, then times tanh' in place
    if ((e = gemm_linear(G(l), w.out[l], nullptr, nullptr, 0, nullptr, wv_t(w.w[l], H), nullptr, b.g[l - 1], B, H,
                         kActNone, nullptr, s)))
      return e;
    hipLaunchKernelGGL(pinn_tanh_grad_kernel, dim3(blocks_of(B * H)), dim3(256), 0, s, b.g[l - 1], t.a[l - 1], B * H,
                       b.g[l - 1]);
  }
  if (grad_state && (e = gemm_linear(b.g[0], H, nullptr, nullptr, 0, nullptr, wv_t(w.w[0], D), nullptr, grad_state, B, D,
                                     kActNone, grad_out, s)))
    return e;
  return hipGetLastError();
}

bool pinn_loss_nx_ok(int nx) { return nx >= 1 && nx <= kFvLdsMaxNx; }

int64_t pinn_loss_ws_bytes(int B, int) { return (int64_t)carve_pinn_loss_ws(B, nullptr).bytes; }

hipError_t launch_pinn_loss(const float *pred, const float *st, const float *sn, int B, int nx, double dt, double dx,
                            double nu, const float *w, const double *pc, float *losses, float *grad_pred, void *ws,
                            hipStream_t s) {
  if (!pinn_loss_nx_ok(nx) || B < 1) return hipErrorInvalidValue;
  const double n1 = (double)B * nx, n3 = 3.0 * n1;
  PinnLossArgs a{};
  a.p = pred, a.s = st, a.sn = sn, a.pc = pc;
  a.B = B, a.nx = nx;
  a.inv_dt = 1.0 / dt;
  a.inv_2dx = 1.0 / (2.0 * dx);
  a.nu_dx2 = nu / (dx * dx);
  for (int k = 0; k < 4; ++k) a.w[k] = (double)w[k];
  a.gd = 2.0 * a.w[0] / n3;
  a.gc = 2.0 * a.w[1] / (dt * n1);
  a.gm = 2.0 * a.w[2] / (dt * n1);
  a.gp = 2.0 * a.w[3] / n1;
  a.inv_n3 = 1.0 / n3;
  a.inv_n1 = 1.0 / n1;
  const LossWs lw = carve_pinn_loss_ws(B, ws);
  a.cnt = lw.cnt;
  a.part = lw.part;
  a.losses = losses;
  a.g = grad_pred;
  // the arrival counter starts every launch at 0 (a memset node, not a kernel)
  if (hipError_t e = hipMemsetAsync(lw.cnt, 0, 16, s)) return e;
  hipLaunchKernelGGL(pinn_loss_kernel, dim3((unsigned)B), dim3(kLossThreads), pinn_loss_lds_bytes(nx), s, a);
  return hipGetLastError();
}

}  // namespace hf
