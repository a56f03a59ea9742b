// Internal declarations shared by the HIP translation units of libhybridflux.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hybridflux.h"

namespace hf {

// Device scratch (workspaces, tapes): every piece starts 256-byte aligned, and
// the one piece of code that cuts a buffer also gives its size.  A layout is a
// function carve_<thing>(shape..., void *base) that takes its pieces from a
// Carve in order and returns their pointers and `bytes`; on a NULL base the
// pointers are NULL and `bytes` is the size query's answer.
inline size_t round256(size_t v) { return (v + 255) & ~size_t(255); }

struct Carve {
  char *base;  // NULL: a size query
  size_t off = 0;
  explicit Carve(void *b) : base(static_cast<char *>(b)) {}
  template <class T>
  T *take(size_t n) {
    T *r = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += round256(sizeof(T) * n);
    return r;
  }
};

// a buffer of one piece, n elements of T
template <class T>
struct OnePiece {
  T *p;
  size_t bytes;
};
template <class T>
inline OnePiece<T> carve_one(size_t n, void *base) {
  Carve c(base);
  T *p = c.take<T>(n);
  return {p, c.off};
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

// Edges bucketed by key (row or col): the CSR's degree, offset, cursor and
// permutation arrays, a sub-layout of every buffer that holds one.
struct EdgeBuckets {
  int *deg, *off, *cur, *perm;
};
inline EdgeBuckets carve_edge_buckets(Carve &c, int64_t N, int64_t E) {
  EdgeBuckets b{};
  b.deg = c.take<int>(N);
  b.off = c.take<int>(N + 1);
  b.cur = c.take<int>(N);
  b.perm = c.take<int>(E);
  return b;
}

// Width of the fused chain kernels: MODEL_CONFIG (src/config.py:19-23) is
// input_dim 4, hidden 128, 4 layers.  16x16x4 f32 MFMA tiles => 8 feature
// tiles of 16 and 32 k-steps of 4 per 128-wide half of a [h ; agg] input.
constexpr int kIn = 4;
constexpr int kH = 128;
constexpr int kNT = kH / 16;
constexpr int kKS = kH / 4;

// Window geometry of the halo-recompute chain kernel (any nx): a wave owns
// 64 consecutive cells; L update layers invalidate L cells at each window
// edge and the readout needs both cells of a face, so faces [L, 62 - L] of
// the window are exact.
constexpr int kWinCells = 64;
// exact faces per window of `cells` cells for L update layers: [L, cells - 2 - L]
// (55 at 64 cells and L = 4, 47 at L = 8)
__host__ __device__ inline int win_faces_of(int layers, int cells = kWinCells) { return cells - 2 * layers - 1; }

// Packed weights (device) for the chain kernels; see capi.cpp pack_chain_*
// for the exact index maps.  The big matrices form ONE stream of chunks,
// consumed in order through an LDS ring (chain_common.h):
//  f32   (v_mfma_f32_16x16x4_f32): 8 KiB chunks, 16 per update layer (4 k-steps
//        each, [h ; agg] input order) + 2 per readout output tile.
//  k32   (v_mfma_f32_16x16x32_{f16,bf16}): per update layer 8 chunks, then one
//        chunk per readout output tile, in the order the cores walk a layer:
//        output pair, then k-block.  f16x3: 16 KiB of (hi, lo) fp16 fragment
//        pairs; bf16: 8 KiB.  (A core may move two chunks at once.)
// Each chunk is [fragment j][lane 64][16 B], so one wave instruction moves 1 KiB.
enum ChainPrec { kPrecF32 = HF_WDTYPE_F32, kPrecBF16 = HF_WDTYPE_BF16, kPrecF16x3 = HF_WDTYPE_F16X3 };
constexpr int kMaxChainLayers = 8;

// Poisson by float64 FFT for power-of-two nx in [kFftMinNx, kFftMaxNx] (fv_poisson.hip).
constexpr int kFftMinNx = 256;
constexpr int kFftMaxNx = 2048;
__host__ __device__ inline bool poisson_uses_fft(int nx) {
  return nx >= kFftMinNx && nx <= kFftMaxNx && (nx & (nx - 1)) == 0;
}
__host__ __device__ inline int poisson_plan_len(int nx) { return poisson_uses_fft(nx) ? 3 * nx : nx; }
// Poisson mode of every FV/Poisson launcher below (pm): HF_POISSON_SPECTRAL
// (the reference's operator; its plan is hf_poisson_coeffs) or
// HF_POISSON_TRIDIAG (opt-in, not the reference's; plan = {dx/2}; one wave's
// cyclic reduction over an LDS row of nx doubles, so nx <= kTriMaxNx).
constexpr int kTriMaxNx = 16384;  // 128 KiB of LDS
bool poisson_mode_ok(int pm, int nx);

__host__ __device__ inline int chain_chunks(int layers, int prec) {
  return prec == kPrecF32 ? 16 * layers + 2 * kNT : 8 * layers + kNT;
}
__host__ __device__ inline int chain_chunk_bytes(int prec) { return prec == kPrecF16x3 ? 16384 : 8192; }
// bf16 streams end with a copy of their first kBF16StreamTail bytes (two 4 KiB units)
constexpr int kBF16StreamTail = 8192;

struct ChainW {
  const void *stream;   // [chain_chunks][chunk]
  const float *win;     // [2][64][4]   input layer A fragments (f32; bf16-rounded in bf16 mode)
  const float *bin;     // [kH]
  const float *bl;      // [L][kH]
  const float *be;      // [kH]
  const float *w2;      // [kH]
  float b2;
  int layers;
  int prec;             // ChainPrec
  int radius;           // stencil radius R of the neighbour mean (1..3; > 1: f32 only); W_b is packed as w / (2R)
};

// Natural-layout float32 weights (device) for the generic-graph path.
struct GraphW {
  const float *w_in, *b_in;        // [H][in], [H]
  const float *w_l, *b_l;          // layer l: w_l + l*lsw [H][2H], b_l + l*lsb [H]
  const float *w_e, *b_e;          // [H][2H], [H]
  const float *w_2, *b_2;          // [H], [1]
  int in_dim, hidden, layers;
  int agg_sum;                     // 1: agg is the neighbour SUM, the 1/deg folded into w_l's W_b half by the caller
                                   // (a radius model's own chain graph, capi.cpp); 0: the mean, sum / max(deg, 1)
  int64_t lsw, lsb;                // per-layer strides (grouped or state-dict order)
};
// Strided weight view for the generic MFMA GEMM (graph.hip):
// weight(o, k) = k < K1 ? w1[o*so + k*si] : w2[o*so + (k-K1)*si].
struct WView {
  const float *w1, *w2;
  int64_t so, si;
};
inline WView wv_rows(const float *W, int K1, int K) { return {W, W + K1, K, 1}; }  // nn.Linear [O][K]
inline WView wv_t(const float *W, int Kf) { return {W, W, 1, Kf}; }              // W^T of [Kf'][Kf]
enum { kActNone = 0, kActRelu = 1, kActTanh = 2 };
// out[m][o] = resid[m][o] + act(b[o] + sum_k weight(o,k) in(m,k)), in(m,k) = [A1[i1(m)] ; A2[i2(m)]][k].
hipError_t gemm_linear(const float *A1, int K1, const int64_t *i1, const float *A2, int K2, const int64_t *i2,
                       WView W, const float *b, float *out, int64_t M, int O, int act, const float *resid,
                       hipStream_t s);
// gw[o][k] = sum_m D[m][o] X[m][k] ([O][K], rows ldw floats apart: ldw > K writes a column
// block of a wider matrix), gb[o] = column sums of D (or NULL); M > 0.  Split-K over the
// rows with the splits summed in a fixed order; part: gemm_wgrad_part_floats(M, O, K) floats.
hipError_t gemm_wgrad(const float *D, int O, const float *X, int K, int64_t M, float *gw, int64_t ldw, float *gb,
                      float *part, hipStream_t s);
int64_t gemm_wgrad_part_floats(int64_t M, int O, int K);
// Fills b (carve_edge_buckets) by key, ascending edge id per bucket (b.off, b.perm); chain_nx > 0: arithmetic buckets.
hipError_t edge_buckets(const int64_t *key, int64_t E, int64_t N, const EdgeBuckets &b, hipStream_t s, int chain_nx = 0,
                        bool by_col = false);

// PureGNN / PINN inference (baselines.hip).
// View of PureGNN's flat float32 parameters in state-dict order.
struct PureW {
  const float *w_in, *b_in;  // [H][in], [H]
  const float *w_l, *b_l;    // layer l at + l*(2H*H + H): [H][2H], [H]
  const float *w_o1, *b_o1;  // [H][H], [H]
  const float *w_o2, *b_o2;  // [3][H], [3]
  int in_dim, H, L;
  int64_t ls;
  const float *w_lp, *w_o1p;  // the one-launch rollout's packed copies: [l][u][P|Q][kb][lane][4], [u][kb][lane][4]
};
PureW pure_view(const float *p, int in_dim, int H, int L);
// shapes of the chain form of PureGNN's layers (tgemm.h EpiMsg): nx | 128, H % 64 == 0
bool pure_chain_ok(int H, int chain_nx, int64_t N);
int64_t pure_gnn_ws_bytes(int H, int64_t N, int64_t E);
hipError_t launch_pure_gnn_forward(const float *params, int in_dim, int H, int L, const float *nf, int64_t N,
                                   const int64_t *ei, int64_t E, int chain_nx, float *delta, void *ws, hipStream_t s);
hipError_t launch_pure_gnn_run(const float *params, int H, int L, const float *state0, float *final_state,
                               const float *x, int B, int nx, int T, float *traj, void *ws, hipStream_t s);
// scratch the rollouts actually use: the packed weights on their one-launch paths (baselines.hip)
int64_t pure_gnn_run_ws_bytes(int H, int B, int nx, int T);
// the one-launch PureGNN rollout also runs with no workspace (on nn.Linear's rows, unpacked)
bool pure_gnn_run_ws_optional(int H, int nx, int T);
int64_t pinn_run_ws_bytes(int D, int H, int64_t B);
hipError_t launch_pinn_forward(const float *params, int D, int H, int L, const float *state, float *out, int64_t B,
                               void *ws, hipStream_t s);
hipError_t launch_pinn_run(const float *params, int D, int H, int L, const float *state0, float *final_state,
                           int64_t B, int T, float *traj, void *ws, hipStream_t s);

// Scored rollouts of the comparison models (baselines.hip pure_score_kernel /
// pinn_score_kernel): the rollout above in one launch that also writes the
// metric series [B][T+1][HF_NUM_METRICS], steps a classical twin of every IC
// when mse [B][T+1][3] is given and scores the model against it per step
// (metrics_cl: the twin's own series).  Fused shapes only (pure_score_fused /
// pinn_score_fused; any T >= 0, nx <= 64); capi.cpp sequences the existing
// kernels on the others.  tri: the twin's Poisson mode is HF_POISSON_TRIDIAG.
bool pure_score_fused(int H, int nx);
bool pinn_score_fused(int D, int H);
hipError_t launch_pure_gnn_score(const float *params, int H, int L, const float *state0, float *final_state,
                                 const float *x, const double *pc, int tri, int B, int nx, int T, float c, float dt,
                                 float nu, float dx2, float *traj, float *metrics, float *mse, float *metrics_cl,
                                 void *ws, hipStream_t s);
hipError_t launch_pinn_score(const float *params, int D, int H, int L, const float *state0, float *final_state,
                             const double *pc, int tri, int64_t B, int T, float c, float dt, float nu, float dx2,
                             float *traj, float *metrics, float *mse, float *metrics_cl, void *ws, hipStream_t s);

// PureGNN training (pure_train.hip): the forward that keeps a tape, the
// backward, and the fused state-MSE loss with its gradient.  layers <= kMaxChainLayers.
int64_t pure_tape_bytes(int H, int L, int64_t N, int64_t E);
int64_t pure_backward_ws_bytes(int in_dim, int H, int L, int64_t N, int64_t E);
hipError_t launch_pure_forward_train(const float *params, int in_dim, int H, int L, const float *nf, int64_t N,
                                     const int64_t *ei, int64_t E, int chain_nx, float *delta, void *tape,
                                     hipStream_t s);
hipError_t launch_pure_backward(const float *params, int in_dim, int H, int L, const float *nf, int64_t N,
                                const int64_t *ei, int64_t E, int chain_nx, const void *tape, const float *grad_delta,
                                float *grad_params, float *grad_nf, void *ws, hipStream_t s);
int64_t state_mse_ws_bytes(int B, int nx);
hipError_t launch_state_mse(const float *delta, const float *st, const float *sn, int B, int nx, float *loss,
                            float *grad_delta, void *ws, hipStream_t s);

// PINN training (pinn_train.hip): the forward that keeps the tanh activations,
// the backward, and the physics loss with its gradient in one launch.
// 2 <= layers <= kMaxChainLayers, B >= 1; the loss needs nx <= kFvLdsMaxNx.
int64_t pinn_tape_bytes(int H, int L, int64_t B);
int64_t pinn_backward_ws_bytes(int D, int H, int L, int64_t B);
hipError_t launch_pinn_forward_train(const float *params, int D, int H, int L, const float *state, int64_t B, float *out,
                                     void *tape, hipStream_t s);
hipError_t launch_pinn_backward(const float *params, int D, int H, int L, const float *state, int64_t B,
                                const void *tape, const float *grad_out, float *grad_params, float *grad_state,
                                void *ws, hipStream_t s);
bool pinn_loss_nx_ok(int nx);
int64_t pinn_loss_ws_bytes(int B, int nx);
hipError_t launch_pinn_loss(const float *pred, const float *st, const float *sn, int B, int nx, double dt, double dx,
                            double nu, const float *w, const double *pc, float *losses, float *grad_pred, void *ws,
                            hipStream_t s);

// View of a flat float32 parameter buffer in state-dict order (the host_params
// order of hf_model_create): update layers interleave weight and bias.
GraphW graph_view_state_dict(const float *p, int in_dim, int hidden, int layers);

// Per-precision launchers (chain_f32.hip, chain_k32.hip = f16x3, chain_bf16.hip); the generic entry
// points below dispatch on ChainW::prec.
hipError_t launch_chain_flux_f32(const ChainW &, const float *, const float *, int64_t, const float *, int, int,
                                 float *, float *, hipStream_t);
hipError_t launch_chain_flux_k32(const ChainW &, const float *, const float *, int64_t, const float *, int, int,
                                 float *, float *, hipStream_t);
hipError_t launch_chain_flux_bf16(const ChainW &, const float *, const float *, int64_t, const float *, int, int,
                                  float *, float *, hipStream_t);
// The f32 core at stencil radius 2, 3 (chain_f32_radius.hip; launch_chain_*_f32 hand over on ChainW::radius > 1).
hipError_t launch_chain_flux_f32_radius(const ChainW &, const float *, const float *, int64_t, const float *, int,
                                        int, float *, float *, hipStream_t);
// Extra outputs of the persistent rollout: a classical twin of every IC
// stepped in the same wave (hf_run_compare), all optional.
struct RolloutExtras {
  float nu = 0.f, dx2 = 1.f;        // classical viscosity and f32(dx*dx)
  float *mse = nullptr;             // [B][T+1][3]; non-null enables the twin
  float *metrics_cl = nullptr;      // [B][T+1][HF_NUM_METRICS]
  int poisson = HF_POISSON_SPECTRAL;  // Poisson mode (pm) of the hybrid step and the twin
};
hipError_t launch_chain_rollout_f32(const ChainW &, const float *, float *, const float *, const double *, int, int,
                                    int, float, float, float *, float *, float *, const RolloutExtras &,
                                    hipStream_t);
hipError_t launch_chain_rollout_f32_radius(const ChainW &, const float *, float *, const float *, const double *,
                                           int, int, int, float, float, float *, float *, float *,
                                           const RolloutExtras &, hipStream_t);
// Cell-split rollout for small batches (chain_f32.hip; f32, nx in {32,48,64}, no classical twin, radius 1).
bool chain_rollout_prefers_cells(const ChainW &, int B, int nx);
hipError_t launch_chain_rollout_cells(const ChainW &, const float *, float *, const float *, const double *, int,
                                      int, int, float, float, float *, float *, float *, int pm, hipStream_t);
hipError_t launch_chain_rollout_k32(const ChainW &, const float *, float *, const float *, const double *, int, int,
                                    int, float, float, float *, float *, float *, const RolloutExtras &,
                                    hipStream_t);
hipError_t launch_chain_rollout_bf16(const ChainW &, const float *, float *, const float *, const double *, int, int,
                                     int, float, float, float *, float *, float *, const RolloutExtras &,
                                     hipStream_t);

// A model set's fused rollout (hf_run_set): one launch of M x G workgroups,
// G the workgroup count of one model's B ICs; each workgroup reads its model's
// ChainW from table[blockIdx.x / G] (device memory, M entries of one prec).
// Model m starts from state0 + m*stride0 (stride0 = 0: shared ICs) and every
// output carries a leading [M] axis.  Needs M*B and M*G within int.
struct ChainSet {
  const ChainW *table;
  int M;
  int prec;
  int64_t stride0;
  int radius;  // the models' common stencil radius
};
hipError_t launch_chain_rollout_set_f32(const ChainSet &, const float *, float *, const float *, const double *, int,
                                        int, int, float, float, float *, float *, float *, const RolloutExtras &,
                                        hipStream_t);
hipError_t launch_chain_rollout_set_f32_radius(const ChainSet &, const float *, float *, const float *,
                                               const double *, int, int, int, float, float, float *, float *,
                                               float *, const RolloutExtras &, hipStream_t);
hipError_t launch_chain_rollout_set_k32(const ChainSet &, const float *, float *, const float *, const double *, int,
                                        int, int, float, float, float *, float *, float *, const RolloutExtras &,
                                        hipStream_t);
hipError_t launch_chain_rollout_set_bf16(const ChainSet &, const float *, float *, const float *, const double *, int,
                                         int, int, float, float, float *, float *, float *, const RolloutExtras &,
                                         hipStream_t);
inline hipError_t launch_chain_rollout_set(const ChainSet &set, const float *state0, float *state_final,
                                           const float *x, const double *pc, int B, int nx, int T, float c, float dt,
                                           float *traj, float *flux_traj, float *metrics, hipStream_t s,
                                           const RolloutExtras &ex) {
  return set.prec == kPrecF32
             ? launch_chain_rollout_set_f32(set, state0, state_final, x, pc, B, nx, T, c, dt, traj, flux_traj,
                                            metrics, ex, s)
             : launch_chain_rollout_set_k32(set, state0, state_final, x, pc, B, nx, T, c, dt, traj, flux_traj,
                                            metrics, ex, s);
}

// Chain flux.  Feature source: AoS node features [B*nx][4] (nf != nullptr)
// or SoA state [B][3][nx] with IC stride ld_state floats + x[nx].
inline hipError_t launch_chain_flux(const ChainW &w, const float *nf, const float *state, int64_t ld_state,
                                    const float *x, int B, int nx, float *flux_edge, float *flux_face,
                                    hipStream_t s) {
  return w.prec == kPrecF32 ? launch_chain_flux_f32(w, nf, state, ld_state, x, B, nx, flux_edge, flux_face, s)
                            : launch_chain_flux_k32(w, nf, state, ld_state, x, B, nx, flux_edge, flux_face, s);
}

// Work of one step of the per-step flux kernel for B ICs of nx cells, in the
// persistent kernel's own units, and how many units one round of its resident
// workgroups takes (hf_run's lanes cut the batch at whole rounds).  Known for
// the bf16 super-window kernel (chain_bf16.hip); per_round = 0 otherwise.
struct FluxWork {
  int64_t units = 0, per_round = 0;
};
FluxWork chain_flux_work(const ChainW &w, int64_t B, int nx);

// Persistent fused rollout for nx in {16,32,48,64}.
inline hipError_t launch_chain_rollout(const ChainW &w, const float *state0, float *state_final,
                                       const float *x, const double *pc, int B, int nx, int T, float c,
                                       float dt, float *traj, float *flux_traj, float *metrics,
                                       hipStream_t s, const RolloutExtras &ex = RolloutExtras()) {
  return w.prec == kPrecF32
             ? launch_chain_rollout_f32(w, state0, state_final, x, pc, B, nx, T, c, dt, traj, flux_traj, metrics,
                                        ex, s)
             : launch_chain_rollout_k32(w, state0, state_final, x, pc, B, nx, T, c, dt, traj, flux_traj, metrics,
                                        ex, s);
}

// Per-step channel MSE between two trajectories [B][T+1][3][nx] -> [B][T+1][3].
hipError_t launch_traj_mse(const float *a, const float *b, int B, int T1, int nx, float *mse, hipStream_t s);
hipError_t launch_rollout_summary(const float *met, const float *mse, const float *met_ref, int B, int T,
                                  float *summary, float *drift, hipStream_t s);

// One FV + Poisson update (any nx).  face_flux != nullptr => hybrid update
// with that F; nullptr => classical (F = n*u, viscosity).  IC strides in floats.
hipError_t launch_fv_step(const float *in, int64_t ld_in, float *out, int64_t ld_out,
                          const float *face_flux, const double *pc, int B, int nx, float c,
                          float dt, float nu, float dx2, float *flux_out, int64_t ld_flux,
                          float *metrics, int64_t ld_metrics, int pm, hipStream_t s);

// Largest nx whose chain and circulant column fit the one-workgroup-per-IC LDS
// plan of fv_poisson.hip (144 KiB of dynamic LDS); beyond it the update and the
// Poisson sum run tiled over global memory.
constexpr int kFvLdsMaxNx = 6144;

// Per-row moments of states [rows][3][nx] (metrics.hip): moments[r] = (e, q) =
// (0.5 (sum u^2 + sum E^2) / nx, sum n / nx) in float64, one wave per row, a
// lane's cells in ascending order and the lanes in a fixed tree.  Any nx >= 1.
hipError_t launch_state_moments(const float *states, int64_t rows, int nx, double *moments, hipStream_t s);

// The energy and charge terms of the unrolled-training _ex calls
// (include/hybridflux.h): L_cons's step term on the predicted state, the sums
// riding the kernels' loss reduction.  ref [B][2] (eref, qref) float64, coef
// [B][2] (ce, cq) float32 out; NULL ConsTerms: the state term alone.
struct ConsTerms {
  float lam_e, lam_q, scale;
  const double *ref;
  float *coef;
};

// The six unrolled-training launchers below all take `bool ex` first: false is
// the plain entry points' kernel instantiation (cons / coef not read), true the
// _ex entry points' (the wider loss row; the energy and charge terms when cons
// / coef is given, and with it NULL the plain instantiation's bits from the
// other kernel).  The shared device helpers are unroll_common.h's.
//
// Unrolled training (unroll.hip): one hybrid step from the FluxGNN's edge flux
// fe [B][2nx] with the step's extras, and its adjoint; spectral Poisson,
// nx <= kFvLdsMaxNx (unroll_nx_ok).  Contiguous [B][3][nx] states.
//  update:  st_next = launch_fv_step(face_flux = 0.5 (fe[i] + fe[nx + i])) bit
//           for bit; nf_next [B*nx][4] = [n', u', E', x] (or NULL); with target
//           [B][3][nx]: loss[0] = scale * sum w_ch (st_next - target)^2, summed
//           in a fixed order through ws (unroll_ws_bytes; w: 3 host floats).
//           ex: loss[4] = (total, state, energy, charge), ws of
//           unroll_ws_bytes_ex with cons.
//  adjoint: g = direct_next + gnf_next[:, 0:3]^T (each or NULL) + 2 w scale
//           (st_next - target) is dL/d st_next; writes g_fe [B][2nx] = dL/d fe
//           and direct [B][3][nx] (or NULL) = the part of dL/d st that does not
//           pass through the FluxGNN.  ex with coef: the seed of u', E' gains
//           coef[b][0] u', coef[b][0] E' (cq is not added: no gradient through
//           the conservative update).
bool unroll_nx_ok(int nx);
int64_t unroll_ws_bytes(int B, int nx);
int64_t unroll_ws_bytes_ex(int B, int nx);
hipError_t launch_unroll_update(bool ex, const float *fe, const float *st, const float *x, const double *pc, int B,
                                int nx, float c, float dt, float *st_next, float *nf_next, const float *target,
                                const float *w, float scale, float *loss, void *ws, const ConsTerms *cons,
                                hipStream_t s);
hipError_t launch_unroll_adjoint(bool ex, const float *st, const float *st_next, const float *target, const float *w,
                                 float scale, const float *direct_next, const float *gnf_next, const double *pc, int B,
                                 int nx, float c, float dt, float *g_fe, float *direct, const float *coef,
                                 hipStream_t s);

// Unrolled training of PureGNN (pure_unroll.hip): the residual update of one
// rollout step from PureGNN's delta [B*nx][3] with the step's extras, and its
// adjoint; any nx >= 1, tiled over cells.  Contiguous [B][3][nx] states.
//  update:  st_next[b][ch][i] = st[b][ch][i] + delta[b*nx+i][ch] (one float32
//           add); nf_next [B*nx][4] = [n', u', E', x] (or NULL); with target
//           [B][3][nx]: loss[0] = scale * sum w_ch (st_next - target)^2, summed
//           in a fixed order through ws (pure_unroll_ws_bytes; w: 3 host floats).
//           ex: loss[4] = (total, state, energy, charge), ws of
//           pure_unroll_ws_bytes_ex with cons.
//  adjoint: gd[b*nx+i][ch] = (2 w_ch scale (st_next - target)[b][ch][i] +
//           gd_next[b*nx+i][ch]) + gnf_next[b*nx+i][ch] (gd_next [B*nx][3],
//           gnf_next [B*nx][4], each or NULL: the term is left out).  ex with
//           coef: the seed gains (cq, ce u', ce E').
bool pure_unroll_shape_ok(int B, int nx);  // B, nx >= 1 and at most 2^31 - 1 tiles of 1024 cells
int64_t pure_unroll_ws_bytes(int B, int nx);
int64_t pure_unroll_ws_bytes_ex(int B, int nx);
hipError_t launch_pure_unroll_update(bool ex, const float *delta, const float *st, const float *x, int B, int nx,
                                     float *st_next, float *nf_next, const float *target, const float *w, float scale,
                                     float *loss, void *ws, const ConsTerms *cons, hipStream_t s);
hipError_t launch_pure_unroll_adjoint(bool ex, const float *st_next, const float *target, const float *w, float scale,
                                      const float *gd_next, const float *gnf_next, int B, int nx, float *gd,
                                      const float *coef, hipStream_t s);

// Unrolled training of PINN (pinn_unroll.hip): the loss term of one rollout
// step and the gradient its hf_pinn_backward takes in; include/hybridflux.h has
// the formulas.  Contiguous [B][3][nx] states, nx <= kFvLdsMaxNx, B >= 1.
//  loss:    losses[5] = (total, data, cont, mom, pois) of pred against target,
//           residuals on (pred, state); phys (3 host floats) NULL: data only,
//           state and pc not read.  ws: pinn_unroll_ws_bytes.  ex: losses[7] =
//           (..., energy, charge), ws of pinn_unroll_ws_bytes_ex with cons.
//  adjoint: grad_out = d term / d pred + d next term / d (state slot) (with
//           phys and pred_next) + grad_state_next (or NULL: left out).  ex with
//           coef: d term / d pred gains (cq, ce p_u, ce p_E).
bool pinn_unroll_nx_ok(int nx);
int64_t pinn_unroll_ws_bytes(int B, int nx);
int64_t pinn_unroll_ws_bytes_ex(int B, int nx);
hipError_t launch_pinn_unroll_loss(bool ex, const float *pred, const float *state, const float *target, int B, int nx,
                                   const float *w, float scale, const float *phys, float phys_scale, double dt,
                                   double dx, double nu, const double *pc, float *losses, void *ws,
                                   const ConsTerms *cons, hipStream_t s);
hipError_t launch_pinn_unroll_adjoint(bool ex, const float *pred, const float *state, const float *target,
                                      const float *pred_next, const float *grad_state_next, int B, int nx,
                                      const float *w, float scale, const float *phys, float phys_scale, double dt,
                                      double dx, double nu, const double *pc, float *grad_out, const float *coef,
                                      hipStream_t s);

// The whole classical rollout (T steps of launch_fv_step's classical update)
// in one launch, states held in registers: FFT nx up to 1024 (fv_run_fused).
// state0 [B] x IC stride ld_s0 floats, state_final [B][3][nx] (may alias
// state0, may be NULL); traj [B][T+1][3][nx] rows 1..T, flux_traj [B][T][nx],
// metrics [B][T+1][4] rows 1..T, each optional; ref + mse (both or neither):
// per-step channel MSE [B][T+1][3] of ref [B][T+1][3][nx] minus this rollout,
// rows 0..T, bit-identical to launch_traj_mse on the recorded trajectory.
bool fv_run_fused(int nx);
hipError_t launch_fv_run(const float *state0, int64_t ld_s0, float *state_final, float *traj, const double *pc, int B,
                         int nx, int T, float c, float dt, float nu, float dx2, float *flux_traj, float *metrics,
                         const float *ref, float *mse, int pm, hipStream_t s);

// Coarse-graining of a fine classical rollout (hf_coarsen_traj's definition:
// r fine cells per coarse cell, S fine steps per coarse step).
// launch_coarsen_state: fine rows S (t0 + k) of tf (ld_f floats per IC) ->
// coarse rows row0 + k of tc (ld_c floats per IC), k < rows, 3 channels.
// launch_coarsen_flux: fine steps S (t0 + k) .. + S - 1 of ff -> coarse flux
// row row0 + k of fc.  launch_fv_run_coarse: launch_fv_run's classical rollout
// over T_c * S fine steps at the fused sizes (fv_run_fused(nx_f)) that stores
// only the coarse rows traj [B][T_c+1][3][nx_f/r], the coarse flux
// [B][T_c][nx_f/r] and the fine state_final (each may be NULL; state0
// contiguous [B][3][nx_f], may alias state_final); equal to the two launches
// above applied to launch_fv_run's trajectory and flux, bit for bit.
hipError_t launch_coarsen_state(const float *tf, int64_t ld_f, float *tc, int64_t ld_c, int B, int rows, int nx_f,
                                int r, int S, int64_t t0, int64_t row0, hipStream_t s);
hipError_t launch_coarsen_flux(const float *ff, int64_t ld_f, float *fc, int64_t ld_c, int B, int rows, int nx_f, int r,
                               int S, int64_t t0, int64_t row0, hipStream_t s);
hipError_t launch_fv_run_coarse(const float *state0, float *state_final, float *traj, const double *pc, int B, int nx_f,
                                int T_c, int r, int S, float c, float dt, float nu, float dx2, float *flux, int pm,
                                hipStream_t s);

// Metrics of a state batch (used for t=0 of non-fused rollouts).
hipError_t launch_state_metrics(const float *st, int64_t ld, int B, int nx, float *metrics,
                                int64_t ld_metrics, hipStream_t s);

hipError_t launch_poisson(const float *n, int ld_n, float *E, int ld_E, const double *pc, int B,
                          int nx, int pm, hipStream_t s);

// Initial conditions from numpy's MT19937 draws (initial_conditions.hip): rows
// n and u of state [B][3][nx] for int64 seeds in [0, 2^32), one wave per seed;
// table [B][HF_IC_TABLE_LEN] or NULL.  ic_draws_host: the same draws for one
// seed on the host (table, gauss [nx]); false: out-of-range seed or nx.
constexpr int kIcMaxNx = 1 << 24;
hipError_t launch_initial_conditions(const int64_t *seeds, int B, int nx, const double *x, float *state, double *table,
                                     hipStream_t s);
bool ic_draws_host(int64_t seed, int nx, double *table, double *gauss);
// Seeded Gaussian state noise (initial_conditions.hip, on the same draw code;
// include/hybridflux.h hf_state_noise): out = in + f32(sig[ch]) * f32(d), one
// wave per sample; rows with sig[ch] == 0 are copied, row E is left to the
// caller's Poisson launch when skip_E.  zero_mean holds g_n in LDS: nx <=
// kNoiseZeroMeanMaxNx.  launch_state_finish, behind the Poisson launch: seal
// (with skip_E) turns the samples the noise kernel marked as failed NaN (their
// n row stayed finite for the solve); nf (or NULL) [B*nx][4] = [n, u, E, x].
// gauss_host: standard_normal(count) of RandomState(seed); false: bad seed or count.
constexpr int kNoiseZeroMeanMaxNx = 6144;
hipError_t launch_state_noise(const int64_t *seeds, int B, int nx, const float *sig, bool zero_mean, bool skip_E,
                              const float *in, float *out, float *noise, hipStream_t s);
hipError_t launch_state_finish(float *state, const float *x, int B, int nx, bool seal, float *nf, hipStream_t s);
bool gauss_host(int64_t seed, int64_t count, double *gauss);

int64_t graph_workspace_bytes(const GraphW &w, int64_t N, int64_t E);
// Training forward (activation tape) and backward, graph_train section of graph.hip.
int64_t graph_tape_bytes(const GraphW &w, int64_t N, int64_t E);
int64_t graph_backward_ws_bytes(const GraphW &w, int64_t N, int64_t E);
hipError_t launch_graph_forward_train(const GraphW &w, const float *nf, int64_t N, const int64_t *ei, int64_t E,
                                      int chain_nx, float *flux, void *tape, hipStream_t s);
hipError_t launch_graph_backward(const GraphW &w, const float *nf, int64_t N, const int64_t *ei, int64_t E,
                                 int chain_nx, const void *tape, const float *grad_flux, float *grad_params, float *grad_nf,
                                 void *ws, hipStream_t s);
// Chain-specialised training path (train_chain.hip): tagged chain graphs
// (chain_nx > 0) with hidden a power of two in [32, 256], in_dim <= 8 and
// N * 2 * hidden + 2 * hidden < 2^31; other graphs and widths take the
// generic CSR path.
bool chain_train_ok(const GraphW &w, int chain_nx, int64_t N);
int64_t chain_tape_bytes(const GraphW &w, int64_t N);
int64_t chain_backward_ws_bytes(const GraphW &w, int64_t N);
hipError_t launch_chain_forward_train(const GraphW &w, const float *nf, int64_t N, int nx, float *flux, void *tape,
                                      hipStream_t s);
hipError_t launch_chain_backward(const GraphW &w, const float *nf, int64_t N, int nx, const void *tape,
                                 const float *grad_flux, float *grad_params, float *grad_nf, void *ws, hipStream_t s);
// Fused training path (chain_f32.hip): FluxGNN(4, 128, L <= 8) on chains of
// nx in {16, 32, 48, 64}.  Forward: the flux kernel's IC-per-wave pass,
// storing the tape (h[l] at h0 + l * hstride, pq) and the ReLU' bits of
// h[0..L-1] (chain_train_mask_bytes); `pack` holds chain_train_pack_bytes(L)
// of device-packed weights.  Backward: the data gradients g[L..0] (g[l] at
// g0 + l * gstride) from the readout's dP / dQ; `bpack` holds
// chain_train_bwd_pack_bytes(L) of transposed weights, packed by the forward's
// launch (the parameters do not change between the two passes of a step).
bool chain_train_fused_ok(const GraphW &w, int nx);
int64_t chain_train_pack_bytes(int layers);
int64_t chain_train_mask_bytes(int layers, int64_t N);
int64_t chain_train_bwd_pack_bytes(int layers);
hipError_t launch_chain_train_fwd_fused(const GraphW &w, const float *nf, int64_t B, int nx, float *fe, float *h0,
                                        int64_t hstride, float *pq, unsigned *mbits, void *pack, void *bpack,
                                        hipStream_t s);
hipError_t launch_chain_train_bwd_fused(const GraphW &w, int64_t B, int nx, float *g0, int64_t gstride,
                                        const unsigned *mbits, const void *bpack, const float *dPQ,
                                        hipStream_t s);
// The ablation loss's single-step terms and d loss / d flux_edge (train_chain.hip).
int64_t ablation_loss_ws_bytes(int B, int nx);
hipError_t launch_ablation_loss(const float *fe, const float *st, const float *ft, const float *sn, int B, int nx,
                                float c, float dx, const float *lam, int roll, float dt, const double *pc, float *loss,
                                float *flux_loss, float *dfe, void *ws, hipStream_t s);
constexpr int kLossMaxRollout = 3;  // rollout energy term in the loss kernels: rollout_steps <= 3
// The trainer's batch gather + chain node features (train_chain.hip).
hipError_t launch_chain_batch_gather(const int64_t *idx, int B, const float *st_all, const float *ft_all,
                                     const float *sn_all, int64_t N, int nx, const float *x, float *st, float *ft,
                                     float *sn, float *nf, hipStream_t s);
// Adam over one flat parameter buffer, step count on the device (optim.hip); _ex: the
// guarded step (clip by the global norm, weight decay, device lr, non-finite skip), with
// the norm's launch when ws (adam_flat_ws_bytes of float64 partials) is given.
hipError_t launch_adam_flat(float *p, const float *g, float *m, float *v, int64_t n, float *step, unsigned *done,
                            float lr, float b1, float b2, float eps, hipStream_t s);
int64_t adam_flat_ws_bytes(int64_t n);
hipError_t launch_adam_flat_ex(float *p, const float *g, float *m, float *v, int64_t n, float *step, unsigned *done,
                               const float *dev_lr, float lr, float b1, float b2, float eps, float wd, float max_norm,
                               int skip, void *ws, float *stats, hipStream_t s);
hipError_t launch_graph_flux(const GraphW &w, const float *nf, int64_t N, const int64_t *ei,
                             int64_t E, float *flux, void *ws, hipStream_t s);

}  // namespace hf
