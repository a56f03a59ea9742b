/*
 * hybridflux.h — C ABI of the MI355X hybrid-rollout engine (libhybridflux.so).
 *
 * Drop-in boundary for the hot path of shanedirksen/gnn-plasma-flux: the
 * per-timestep loop  FluxGNN message passing on the periodic 1-D chain
 * -> flux symmetrisation -> finite-volume continuity + Burgers update ->
 * spectral Poisson solve.  The reference has no FFI of its own (it is pure
 * Python); each entry point below names the reference function it replaces
 * (paths relative to the reference root).  The Python host layer
 * (gnn-plasma-flux_amd/hybridflux) binds these through ctypes; INTEGRATION.md
 * shows the binding.
 *
 * Conventions
 *  - Every pointer named dev_* is a device (HBM) pointer; host_* are host.
 *  - Layouts: state [B][3][nx] float32 (n,u,E per IC, channel-major, the
 *    reference's [3,nx] per IC); node features [N][in_dim] float32 (AoS, as
 *    FluxGNN.forward receives them); edge fluxes [B][2*nx] in the reference
 *    edge order (edges i->i+1 first, then i+1->i).
 *  - Work is enqueued on `stream` (a hipStream_t, NULL = default stream) and
 *    is asynchronous: nothing here synchronises the host.
 *  - Return 0 on success, a negative HF_E* code on failure; the message is
 *    available from hf_last_error() (thread-local).  Nothing throws across
 *    the ABI.  There is NO CPU fallback: without a usable gfx950 device every
 *    compute entry point fails with HF_EHIP.
 *  - Ownership: the caller owns every state/flux/trajectory/metric buffer.
 *    A model handle owns only its packed, read-only device weights, so
 *    concurrent calls on one handle from different streams are safe.
 */
#ifndef HYBRIDFLUX_H
#define HYBRIDFLUX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HF_OK 0
#define HF_EINVAL (-1)      /* bad argument (shape, NULL pointer, size)        */
#define HF_EUNSUPPORTED (-2)/* configuration this build does not implement    */
#define HF_EHIP (-3)        /* HIP runtime error (no device, launch failure)  */
#define HF_ENOMEM (-4)      /* device allocation failed                       */

#define HF_WDTYPE_F32 0     /* weights and arithmetic in float32 (parity mode) */
#define HF_WDTYPE_BF16 1    /* bf16 MLP weights/activations, f32 accumulate    */
#define HF_WDTYPE_F16X3 2   /* fp32-accurate: fp16 hi+lo split of weights and
                               activations, 3 MFMA products, f32 accumulate   */

/* Number of per-(IC, step) rollout metrics written by hf_run / hf_step /
 * hf_run_compare / hf_traj_metrics:
 * [0] energy 0.5*mean(u^2+E^2)   (scripts/evaluation/evaluate_all.py:135,
 *                                  evaluate_long_rollout.py:38-42)
 * [1] charge mean(n)              (evaluate_all.py:141)
 * [2] 1.0 if every state value is finite else 0.0
 *                                 (evaluate_long_rollout.py:57-60)
 * [3] max |n-1| over the chain (NaN when [2] is 0; no reference counterpart).
 * Sums are float64, rounded to float32 once. */
#define HF_NUM_METRICS 4

/* Per-IC rollout summary written by hf_rollout_summary:
 * [0] exploded_at: first step t >= 1 whose state is not finite, -1 if none
 *     (evaluate_long_rollout.py:53-66)
 * [1] actual_steps: exploded_at - 1, or T (evaluate_long_rollout.py:74)
 * [2] final energy drift |e[a] - e[0]|, a = actual_steps
 *     (evaluate_long_rollout.py:72; evaluate_all.py:137,157)
 * [3] final charge drift |q[a] - q[0]| (evaluate_all.py:143,158)
 * [4] final_mse = mse_total[T], mse_total = mse_n + mse_u + mse_E
 *     (evaluate_all.py:132,155); NaN without an MSE series
 * [5] mean_mse = mean over t = 0..T of mse_total (evaluate_all.py:156,
 *     evaluate_multi_ic.py:91-94); NaN without an MSE series
 * [6], [7] final energy / charge drift of the reference (classical) series
 *     at T (energy_drift_true, charge_drift_true); NaN without one. */
#define HF_NUM_SUMMARY 8

typedef struct hf_model *hf_model_t;

/* Library version string, "hybridflux <ver> gfx950 src:<16 hex>": the hex is a
 * sha256 prefix of the sources, headers and Makefile the library was built
 * from, so a record that prints it names the exact sources that ran. */
const char *hf_version(void);

/* Thread-local message describing the last failure on this thread. */
const char *hf_last_error(void);

/* Number of visible HIP devices (0 when none); never fails. */
int hf_device_count(void);

/*
 * Replaces: FluxGNN.__init__ + load_state_dict (src/flux_gnn.py:11-38,
 * src/hybrid_solver.py:22-28).
 * host_params: every parameter of the reference state dict, float32,
 * concatenated in this order (row-major, shapes as nn.Linear stores them):
 *   input_mlp.0.weight [H][in_dim], input_mlp.0.bias [H],
 *   for l in 0..layers-1: update_mlps.l.0.weight [H][2H], update_mlps.l.0.bias [H],
 *   edge_mlp.0.weight [H][2H], edge_mlp.0.bias [H],
 *   edge_mlp.2.weight [1][H], edge_mlp.2.bias [1].
 * The handle packs them into the MFMA fragment order of the fused chain
 * kernels (when in_dim==4 && H==128) and keeps the natural layout for the
 * generic-graph path (always float32).  wdtype selects the chain kernels'
 * MFMA arithmetic: HF_WDTYPE_F32 (v_mfma_f32_16x16x4_f32, exact f32),
 * HF_WDTYPE_F16X3 (v_mfma_f32_16x16x32_f16 on a two-term fp16 split of both
 * operands, 3 products: fp32-level accuracy at ~5x the f32 MFMA rate) or
 * HF_WDTYPE_BF16 (bf16 weights and activations, config 4).
 */
int hf_model_create(const float *host_params, int in_dim, int hidden, int layers,
                    int wdtype, hf_model_t *out);
/*
 * hf_model_create with a real stencil radius.  Replaces: nothing the reference
 * runs: its radius names a checkpoint (src/hybrid_solver.py:32) and its graph
 * is always the ±1 chain (src/graph_constructor.py:34-38).
 * A model of radius R (1..3) runs FluxGNN.forward on the radius-R chain graph
 * in every fused chain entry point (hf_chain_flux, hf_step, hf_run,
 * hf_run_compare, the model-set calls): per IC a block of 2*R*nx edges, for
 * r = 1..R in order the nx edges i -> (i+r) mod nx, then the nx edges
 * (i+r) mod nx -> i; the update layers' mean runs over the 2R neighbours,
 * summed in the order ((((h[i+1] + h[i-1]) + h[i+2]) + h[i-2]) + h[i+3]) +
 * h[i-3] (a sequential index_add_ over that edge list).  The parameters are
 * those of radius 1 (same host_params).  The solver uses only the first 2nx
 * fluxes of a block (the ±1 edges, F_i = 0.5 (fe[i] + fe[nx+i])), and those
 * are what hf_chain_flux writes: dev_flux_edge stays [B][2nx].  The 1/deg is
 * packed into W_b as float32(w / (2R)): exact for R = 1, 2; R = 3 rounds each
 * weight once instead of each mean.  A model of radius R > 1 needs
 * nx >= 2R + 1 (no repeated edge): HF_EINVAL from every entry point that
 * takes it otherwise (radius-1 models take every nx they always took).
 * hf_model_create is this call with radius 1.  radius outside 1..3:
 * HF_EINVAL; radius > 1 with wdtype != HF_WDTYPE_F32, or on a model that is
 * not chain-capable (in_dim 4, hidden 128, layers <= 8): HF_EUNSUPPORTED; all
 * three before any device call.  Small batches of a radius > 1 model run the
 * IC-per-wave kernels (the cell-split kernels are radius 1): same values.
 * hf_graph_flux ignores the radius: the caller's edge list is the graph.
 */
int hf_model_create_ex(const float *host_params, int in_dim, int hidden, int layers,
                       int wdtype, int radius, hf_model_t *out);
/* The model's stencil radius (1..3); 0 for NULL. */
int hf_model_radius(hf_model_t model);
/*
 * The weight stream hf_model_create_ex packs for the fused chain kernels of a
 * chain-capable model (in_dim 4, hidden 128, layers <= 8), on the HOST: no
 * device is touched (what the host-sanitized tests/native/radius_sanitize.cpp
 * checks).  Returns the stream's size in bytes; with stream_out == NULL that
 * is all it does, otherwise it writes the stream into stream_out, which must
 * hold stream_bytes >= that size.  -1: layers outside 0..8, radius outside
 * 1..3, an unknown wdtype, radius > 1 with wdtype != HF_WDTYPE_F32, NULL
 * host_params, or a stream_out that is too small.
 */
int64_t hf_chain_pack_host(const float *host_params, int layers, int wdtype, int radius,
                           void *stream_out, int64_t stream_bytes);
void hf_model_destroy(hf_model_t model);
/* Total float count host_params must hold for these dimensions. */
int64_t hf_model_param_count(int in_dim, int hidden, int layers);

/*
 * Replaces: FluxGNN.forward (src/flux_gnn.py:40-67) applied to the batched
 * chain graph of build_chain_graph (src/graph_constructor.py:6-39).
 * dev_node_features [B*nx][4]; dev_flux_edge [B][2nx] (may be NULL);
 * dev_flux_face [B][nx] = 0.5*(edge i + edge nx+i) (may be NULL;
 * src/hybrid_solver.py:45-48).  Any nx >= 1.
 */
int hf_chain_flux(hf_model_t model, const float *dev_node_features, int B, int nx,
                  float *dev_flux_edge, float *dev_flux_face, void *stream);

/*
 * Replaces: FluxGNN.forward on an ARBITRARY graph (examples/smoke_test.py:45-56
 * calls it with a random edge_index).  dev_edge_index [2][E] int64.
 * dev_workspace must hold hf_graph_workspace_bytes(model, N, E) bytes.
 */
int64_t hf_graph_workspace_bytes(hf_model_t model, int64_t N, int64_t E);
int hf_graph_flux(hf_model_t model, const float *dev_node_features, int64_t N,
                  const int64_t *dev_edge_index, int64_t E, float *dev_flux,
                  void *dev_workspace, void *stream);

/*
 * FluxGNN.forward of a radius-R model (hf_model_create_ex) on ITS OWN graph:
 * dev_edge_index [2][E], E = 2*R*B*nx, is the radius-R chain graph of B chains
 * of nx cells in the order hf_model_create_ex documents (the caller declares
 * it; graph_constructor.chain_edge_index(nx, B, radius=R) builds it).  Replaces:
 * nothing the reference runs (its graph is always the +-1 chain).  Writes all
 * E fluxes, the long edges' too, through the generic-graph kernels with the
 * fused kernels' arithmetic: the neighbour SUM in edge-list order times W_b
 * packed as float32(w / (2R)), where hf_graph_flux forms the reference's mean
 * (float32 sum / degree, one rounding per mean).  The two agree bit for bit for
 * R <= 2 and to a rounding for R = 3; this call's first 2nx fluxes per IC are
 * hf_chain_flux's definition.  For a radius-1 model it is hf_graph_flux.
 * Workspace: hf_graph_workspace_bytes(model, B*nx, E).  nx < 2R + 1: HF_EINVAL.
 */
int hf_graph_flux_radius(hf_model_t model, const float *dev_node_features, int B, int nx,
                         const int64_t *dev_edge_index, float *dev_flux, void *dev_workspace, void *stream);

/*
 * Training: FluxGNN.forward + autograd backward on any
 * graph (src/flux_gnn.py:40-67 under loss.backward() in
 * scripts/training/train_ablation.py:120-206).  Weights are read from a DEVICE
 * float32 buffer dev_params in the host_params order of hf_model_create
 * (state-dict order), so an optimizer can update them in place between steps.
 *
 * hf_graph_forward_train writes dev_flux[E] (as hf_graph_flux) and an
 * activation tape (hf_graph_tape_bytes) that hf_graph_backward consumes.
 * hf_graph_backward writes dL/dparams (overwriting, same layout as
 * dev_params, hf_model_param_count floats) and, when dev_grad_node_features
 * is not NULL, dL/dnode_features [N][in_dim].  dev_grad_flux is dL/dflux [E].
 * dev_params must be unchanged since the hf_graph_forward_train that wrote
 * the tape: the tape holds weights packed by that forward (and the backward
 * multiplies by dev_params as the forward read them), so the optimizer step
 * comes after hf_graph_backward; with parameters changed in between, the
 * gradients are silently wrong.
 * Weight gradients are split-K sums reduced in a fixed order: bitwise
 * deterministic for a given N, E.  chain_nx > 0 declares that edge_index is
 * N/chain_nx disjoint periodic chains of chain_nx cells in build_chain_graph
 * order (src/graph_constructor.py:34-38, E == 2N): with hidden a power of two
 * in [32, 256], in_dim <= 8 and N * 2 * hidden + 2 * hidden < 2^31 the chain
 * training path runs (the aggregation as
 * a stencil inside the GEMM operand loads, the edge readout split into
 * per-node P/Q GEMMs, f32 MFMA GEMMs throughout); otherwise the edge buckets
 * are formed arithmetically instead of by the count/scan/fill CSR build.  0
 * for any other graph.  chain_nx > 0 declares radius-1 chains: a radius-R
 * chain graph (hf_model_create_ex, E == 2*R*N) passes chain_nx = 0 and runs the
 * generic kernels, which handle any graph.
 */
int64_t hf_graph_tape_bytes(int in_dim, int hidden, int layers, int64_t N, int64_t E);
int64_t hf_graph_backward_workspace_bytes(int in_dim, int hidden, int layers, int64_t N, int64_t E);
int hf_graph_forward_train(const float *dev_params, int in_dim, int hidden, int layers,
                           const float *dev_node_features, int64_t N, const int64_t *dev_edge_index,
                           int64_t E, int chain_nx, float *dev_flux, void *dev_tape, void *stream);
int hf_graph_backward(const float *dev_params, int in_dim, int hidden, int layers,
                      const float *dev_node_features, int64_t N, const int64_t *dev_edge_index, int64_t E,
                      int chain_nx, const void *dev_tape, const float *dev_grad_flux, float *dev_grad_params,
                      float *dev_grad_node_features, void *dev_workspace, void *stream);

/*
 * Replaces: the single-step terms of the reference trainer's ablation loss
 * (scripts/training/train_ablation.py:120-170: flux MSE, state MSE of the
 * finite-volume continuity update, Poisson MSE, charge and one-step energy
 * terms), batched over B samples as hybridflux.training.ablation_loss does.
 * dev_flux_edge [B][2nx] (FluxGNN output), dev_state_t / dev_state_next
 * [B][3][nx], dev_flux_t [B][nx]; c = f32(dt/dx), dx = f32(dx); lam[4] =
 * lambda_state, lambda_poisson, lambda_charge, lambda_energy_one; dev_c the
 * Poisson plan.  Writes dev_loss[0] = loss, dev_flux_loss[0] = the flux MSE
 * term and dev_dflux_edge
 * [B][2nx] = d loss / d flux_edge (the Poisson and energy terms go through a
 * detached solve, as in the reference, and the charge term's gradient is
 * identically 0).  dev_workspace: hf_ablation_loss_workspace_bytes(B, nx).
 */
int64_t hf_ablation_loss_workspace_bytes(int B, int nx);
int hf_ablation_loss(const float *dev_flux_edge, const float *dev_state_t, const float *dev_flux_t,
                     const float *dev_state_next, int B, int nx, float c, float dx, const float *lam,
                     const double *dev_c, float *dev_loss, float *dev_flux_loss, float *dev_dflux_edge,
                     void *dev_workspace, int64_t workspace_bytes, void *stream);

/*
 * Replaces: the whole per-sample loss of the reference trainer, the
 * multi-step rollout energy term included (scripts/training/
 * train_ablation.py:120-206, the 'full' and 'rollout_only' configs).
 * hf_ablation_loss plus lam[4] = lambda_energy_multi and rollout_steps = K,
 * dt = f32(dt): adds lam[4] * mean_{k<K, b} (e_k - e_0)^2, e_k = 0.5 mean(u_k^2)
 * (:172-206), when K > 0 and lam[4] > 0.  The energies use u_0..u_{K-1} only,
 * and u is advanced with the sample's E (k = 0) and then the detached Poisson
 * E of the previous n (:193-200); for K <= 3 that is u_0, u_1 and u_2 with E_1
 * = E(n') of the main forward's n' (the rollout's first forward is the same
 * model on the same state), so no further model forward reaches the loss and
 * the term is formed here from the inputs alone.  It carries no gradient (u
 * does not depend on the parameters), so dev_dflux_edge is hf_ablation_loss's.
 * K > 3 with lam[4] > 0 is HF_EUNSUPPORTED (later energies need forwards on
 * later states: pass lam[4] = 0 and add the term from them).  hf_ablation_loss
 * is this call with lam[4] = 0, K = 0.  Same workspace.
 */
int hf_ablation_loss_ex(const float *dev_flux_edge, const float *dev_state_t, const float *dev_flux_t,
                        const float *dev_state_next, int B, int nx, float c, float dx, const float *lam,
                        int rollout_steps, float dt, const double *dev_c, float *dev_loss, float *dev_flux_loss,
                        float *dev_dflux_edge, void *dev_workspace, int64_t workspace_bytes, void *stream);

/*
 * Replaces: one training batch of the reference trainer (its dataset of
 * (state_t, flux_t, state_next) triples indexed by a DataLoader batch,
 * scripts/training/train_ablation.py:27-44) and the batch's chain node
 * features (src/graph_constructor.py:6-39 build_chain_graph: [n, u, E, x] per
 * cell, batched), in one pass.  dev_idx [B] int64 sample indices (negative
 * ones wrap once, as torch indexing; beyond [-N, N) they are clamped);
 * dataset dev_state_t_all / dev_state_next_all [N][3][nx], dev_flux_t_all
 * [N][nx]; dev_x [nx].  Writes dev_state_t / dev_state_next [B][3][nx],
 * dev_flux_t [B][nx], dev_node_features [B*nx][4].
 */
int hf_chain_batch_gather(const int64_t *dev_idx, int B, const float *dev_state_t_all,
                          const float *dev_flux_t_all, const float *dev_state_next_all, int64_t N, int nx,
                          const float *dev_x, float *dev_state_t, float *dev_flux_t, float *dev_state_next,
                          float *dev_node_features, void *stream);

/*
 * Replaces: the reference trainer's optimizer step (torch.optim.Adam,
 * scripts/training/train_ablation.py:208-209; weight decay 0, no amsgrad) on
 * one flat float32 parameter buffer of n values, in one launch.  dev_step: the
 * step count (float, on the device; read, then incremented by the call, so a
 * captured graph replays it); dev_done: one unsigned, 0 before the first call
 * (the call leaves it 0).  Update per value: m = b1 m + (1 - b1) g, v = b2 v +
 * (1 - b2) g^2, p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
 */
int hf_adam_flat(float *dev_params, const float *dev_grads, float *dev_exp_avg, float *dev_exp_avg_sq, int64_t n,
                 float *dev_step, unsigned *dev_done, float lr, float beta1, float beta2, float eps, void *stream);

/*
 * The guarded optimizer step.  Replaces: torch.nn.utils.clip_grad_norm_ +
 * torch.optim.AdamW + a GradScaler-style skip of a step whose gradient is not
 * finite (a multi-tensor norm, a multi-tensor scale, the update and a host
 * read of the norm per step) around hf_adam_flat, by at most two launches and
 * no host synchronisation, so a captured training step keeps all of it.
 *
 * Launch 1 (made only with a workspace): the sum of g[i]^2 in float64, one
 * partial per workgroup into dev_ws.  The partition is hf_adam_flat's (256
 * threads; ceil(n / 1024) workgroups, 2048 at most): workgroup b's thread t
 * adds the squares of g[(b + k W) 256 + t], k = 0, 1, ... (W workgroups) in
 * ascending k, and the 256 thread sums are added by a halving tree (sum[t] +=
 * sum[t + 128], then t + 64, ..., t + 1).  Launch 2: every workgroup adds the W partials --
 * thread t those at t, t + 256, ... in ascending order, then the same tree --
 * so every workgroup holds the same bits, and two calls on the same gradient
 * give the same norm.  Then, in float32 unless stated:
 *   norm = (float)sqrt(sum),  coef = min(max_norm / (norm + 1e-6f), 1)
 *   skipped = skip_nonfinite and norm is inf or NaN: nothing is written to
 *     dev_params, dev_exp_avg, dev_exp_avg_sq or dev_step
 *   otherwise per value: g' = g coef (g itself when coef == 1: an unclipped
 *     step is bit-equal to one without clipping), p = p (1 - lr wd) when wd !=
 *     0, then hf_adam_flat's update with g' and that p, bit for bit (c1 = 1.0f
 *     - beta1, c2 = 1.0f - beta2, the bias corrections from float64 pow).
 * lr is dev_lr[0] when dev_lr is not NULL (a device float a scheduler rewrites
 * between replays of a captured step), the by-value lr otherwise.  max_norm:
 * INFINITY = no clipping.  dev_step advances except on a skipped step;
 * dev_done as for hf_adam_flat (left 0, skipped or not).  dev_stats
 * [HF_OPT_NUM_STATS] or NULL, written by the last workgroup to finish: (norm
 * before clipping, coef applied (0 on a skipped step), skipped 0/1, skipped
 * steps so far); the last one is read and incremented, so zero the buffer
 * before the first step and hand the same one to every step.
 *
 * dev_ws: hf_adam_flat_workspace_bytes(n) bytes (a multiple of 8, monotone in
 * n; -1 for n < 0), 8-byte aligned.  It may be NULL only when max_norm is
 * INFINITY, skip_nonfinite is 0 and dev_stats is NULL: then no norm launch is
 * made and the call is hf_adam_flat with weight decay and the device lr.
 * HF_EINVAL: n < 0, a NULL pointer with n > 0 (dev_lr, dev_stats and, as said,
 * dev_ws may be NULL), max_norm <= 0 or NaN, weight_decay < 0 or NaN, a missing
 * workspace.  n == 0 is HF_OK without a launch.
 */
#define HF_OPT_NUM_STATS 4
int64_t hf_adam_flat_workspace_bytes(int64_t n);
int hf_adam_flat_ex(float *dev_params, const float *dev_grads, float *dev_exp_avg, float *dev_exp_avg_sq, int64_t n,
                    float *dev_step, unsigned *dev_done, const float *dev_lr, float lr, float beta1, float beta2,
                    float eps, float weight_decay, float max_norm, int skip_nonfinite, void *dev_ws,
                    float *dev_stats, void *stream);

/*
 * Unrolled training: FluxGNN differentiated through K hybrid solver steps.
 * Replaces: the torch ops a user would put around FluxGNN's autograd Function
 * to train through the solver's feedback loop n -> E -> u -> node features
 * (src/hybrid_solver.py:45-63 under autograd: torch.roll for the two upwind
 * differences, torch.fft for a differentiable Poisson solve, the MSE against
 * the classical trajectory), dozens of small launches per unrolled step, by
 * one launch per forward step and one per backward step around
 * hf_graph_forward_train / hf_graph_backward.  The reference trains one step
 * only (its rollout term carries no gradient, hf_ablation_loss_ex above).
 *
 * Step k maps s_k = (n, u, E) [B][3][nx] to s_{k+1} with fe = FluxGNN([n, u, E,
 * x]) [B][2nx] and c = f32(dt/dx), dt = f32(dt):
 *   F_i = 0.5 (fe[i] + fe[nx+i]),  n'_i = n_i - c (F_i - F_{i-1}),
 *   u'_i = u_i - c (u_i^2/2 - u_{i-1}^2/2) + dt E_i,  E' = P(n' - 1)
 * (periodic indices; P the spectral operator of dev_plan = hf_poisson_coeffs),
 * and the loss is L = (1/K) sum_k mean_{b,ch,i} w_ch (s_k - s*_k)^2, k = 1..K.
 *
 * hf_unroll_update: one forward step from dev_flux_edge.  Writes dev_state_next
 * (bit-identical to hf_step's finite-volume update given the same face flux:
 * the same device functions) and, when not NULL, dev_node_features_next
 * [B*nx][4] = [n', u', E', x], the next step's FluxGNN input.  With dev_target
 * [B][3][nx] (else NULL: no loss) it also writes dev_loss[0] = loss_scale *
 * sum_{b,ch,i} weights[ch] (s' - target)^2 (weights: 3 HOST floats;
 * loss_scale = 1 / (K 3 B nx) gives the step's term of L): float64 partials
 * per IC through dev_workspace (hf_unroll_workspace_bytes(B, nx); the call
 * zeroes its arrival counter itself with a memset node), summed in IC order by
 * the last workgroup to arrive, no float atomics: two calls give the same bits.
 *
 * hf_unroll_adjoint: the adjoint of that step.  The total gradient of L with
 * respect to s_{k+1} is g = dev_direct_next + dev_grad_nf_next[:, 0:3]^T +
 * 2 weights loss_scale (dev_state_next - dev_target): the direct part this
 * call wrote for step k+1 and hf_graph_backward's dL/dnode_features of step
 * k+1 ([B*nx][4]; column 3, dL/dx, is not used), each NULL at the last step
 * (and both NULL at every step for the pushforward form, which cuts the state
 * gradient between steps).  With a = g_n, b = g_u, e = g_E and a~ = a + P^T e
 * = a - P e (P is an antisymmetric circulant with zero row sums; e goes
 * through the operator as it is, with no n - 1 subtraction):
 *   dev_grad_flux_edge[i] = dev_grad_flux_edge[nx+i] = -0.5 c (a~_i - a~_{i+1})
 *   dev_direct = (a~_i,  b_i - c u_i (b_i - b_{i+1}),  dt b_i)   [B][3][nx]
 * with u of dev_state (s_k); dev_direct may be NULL (step 0).  dL/ds_k is then
 * dev_direct + dL/dnode_features of step k (+ the seed of s_k for k >= 1, which
 * the next call adds).  Every value is computed by one thread in a fixed
 * order.
 *
 * Kernels: power-of-two nx in [256, 2048] one wave per pair of ICs (the
 * float64 FFT passes); every other nx <= 6144 one 256-thread workgroup per IC
 * with the circulant column and the rows in LDS.  Before any device call: NULL
 * required pointers, B < 1, nx < 1, aliased states or a workspace_bytes too
 * small return HF_EINVAL (hf_unroll_workspace_bytes: -1); nx > 6144 and
 * HF_POISSON_TRIDIAG return HF_EUNSUPPORTED.
 */
int64_t hf_unroll_workspace_bytes(int B, int nx);
int hf_unroll_update(const float *dev_flux_edge, const float *dev_state, const float *dev_x, const double *dev_plan,
                     int poisson_mode, int B, int nx, float c, float dt, float *dev_state_next,
                     float *dev_node_features_next /* or NULL */, const float *dev_target /* or NULL */,
                     const float *weights, float loss_scale, float *dev_loss, void *dev_workspace,
                     int64_t workspace_bytes, void *stream);
int hf_unroll_adjoint(const float *dev_state, const float *dev_state_next, const float *dev_target,
                      const float *weights, float loss_scale, const float *dev_direct_next /* or NULL */,
                      const float *dev_grad_nf_next /* or NULL */, const double *dev_plan, int poisson_mode, int B,
                      int nx, float c, float dt, float *dev_grad_flux_edge, float *dev_direct /* or NULL */,
                      void *stream);

/*
 * The reference's other rollout models, inference.
 * dev_params: every parameter, float32, state-dict order, on the device.
 *
 * PureGNN (scripts/training/train_pure_gnn.py:35-76): input_mlp.0 [H][in],
 * update_mlps.l.0 [H][2H] (+bias) for each layer, output_mlp.0 [H][H],
 * output_mlp.2 [3][H] (+biases); tanh activations, residual message passing.
 * hf_pure_gnn_forward = PureGNN.forward(node_features [N][in], edge_index
 * [2][E]) -> delta [N][3]; chain_nx as for hf_graph_forward_train.
 * hf_pure_gnn_run = the rollout of scripts/evaluation/evaluate_multi_ic.py:45-66
 * (state <- state + delta, node features [n,u,E,x]) for B ICs on chains of nx
 * cells: state0/final [B][3][nx], traj [B][T+1][3][nx] or NULL; x [nx].
 * Workspace: hf_pure_gnn_workspace_bytes(H, N, E) for hf_pure_gnn_forward;
 * hf_pure_gnn_run_workspace_bytes(H, B, nx, T) for hf_pure_gnn_run.  The
 * rollout is ONE launch for all T steps for nx in {16, 32, 48, 64} with H in
 * {64, 128} (one IC per workgroup, activations in LDS); its workspace holds a
 * packed copy of the message/output weights made at the start of the call (the
 * copy for up to 8 layers; with more layers, or with dev_workspace == NULL, the
 * launch reads nn.Linear's rows in place, slower).  Otherwise, on chains whose nx divides 128 with H a multiple of 64,
 * each message layer is one f32 MFMA GEMM that forms the messages and the
 * residual in its epilogue (csrc/tgemm.h EpiMsg); other shapes run the generic
 * linear + gather kernels.
 *
 * PINN (scripts/training/train_pinn.py:36-61): net.0 [H][D], (layers-2) x
 * [H][H], net.last [D][H] (+biases), tanh between; out = state + net(state)
 * on states flattened to D = 3*nx.  hf_pinn_run = evaluate_multi_ic.py:70-83
 * for B ICs: state0/final [B][D], traj [B][T+1][D] or NULL.  The reference's
 * shape (D = 192, H = 256, 2 <= layers <= 8) runs as ONE launch for all T steps
 * (16 ICs per workgroup, activations in LDS; hf_pinn_forward is its T = 1),
 * whose workspace holds a packed copy of the weights made at the start of the
 * call (hf_pinn_workspace_bytes: the copy for the largest layer count, 8);
 * other shapes run per-layer GEMMs through the workspace.  B = 0 or T = 0
 * needs none.  ABI note (round 4): hf_pinn_run / hf_pinn_forward require the
 * workspace whenever hf_pinn_workspace_bytes > 0 (a NULL workspace is
 * HF_EINVAL; it used to be accepted); hf_pure_gnn_run accepts NULL on its
 * one-launch shapes.
 */
int64_t hf_pure_gnn_param_count(int in_dim, int hidden, int layers);
int64_t hf_pure_gnn_workspace_bytes(int hidden, int64_t N, int64_t E);
int64_t hf_pure_gnn_run_workspace_bytes(int hidden, int B, int nx, int T);
int hf_pure_gnn_forward(const float *dev_params, int in_dim, int hidden, int layers,
                        const float *dev_node_features, int64_t N, const int64_t *dev_edge_index, int64_t E,
                        int chain_nx, float *dev_delta, void *dev_workspace, void *stream);
int hf_pure_gnn_run(const float *dev_params, int hidden, int layers, const float *dev_state0,
                    float *dev_final, const float *dev_x, int B, int nx, int T, float *dev_traj,
                    void *dev_workspace, void *stream);

/*
 * PureGNN training (scripts/training/train_pure_gnn.py:59-76 under
 * batch_loss.backward(), :100-151), mirroring hf_graph_forward_train /
 * hf_graph_backward.  dev_params and dev_grad_params are flat float32 device
 * buffers of hf_pure_gnn_param_count values in state-dict order (above);
 * layers <= 8, N >= 1.  chain_nx as for hf_graph_forward_train: tagged chains
 * with chain_nx dividing 128 and hidden a multiple of 64 run on the f32 MFMA
 * GEMMs of csrc/tgemm.h, every other graph, width or chain length on the
 * generic kernels (dev_edge_index must lie in [0, N): it is not checked here).
 *
 * hf_pure_gnn_forward_train writes dev_delta [N][3], bit-identical to
 * hf_pure_gnn_forward, and a tape (hf_pure_gnn_tape_bytes: h_0..h_L, the
 * output_mlp's hidden layer and every message) that hf_pure_gnn_backward
 * consumes.  hf_pure_gnn_backward reads dev_grad_delta = dL/ddelta [N][3] and
 * writes dL/dparams (overwriting) and, when dev_grad_node_features is not
 * NULL, dL/dnode_features [N][in_dim]; workspace
 * hf_pure_gnn_backward_workspace_bytes.  dev_params must be unchanged between
 * the forward that wrote the tape and the backward (the backward multiplies
 * by the weights the forward used), so the optimizer step comes after it.
 * Every sum runs in a fixed order (the messages of a node in ascending edge
 * order, split-K weight gradients reduced in split order, no atomics): two
 * calls on the same inputs give the same bits.
 *
 * hf_state_mse: the trainer's loss (:134-141) for a batch in one pass.
 * dev_delta [B*nx][3], dev_state_t / dev_state_next [B][3][nx]; writes
 * dev_loss[0] = mean((state_t^T + delta - state_next^T)^2) over all 3 B nx
 * values (= the mean over samples of the per-sample means) and dev_grad_delta
 * [B*nx][3] = 2 (pred - target) / (3 B nx), by a two-stage reduction in a
 * fixed order.  dev_workspace: hf_state_mse_workspace_bytes(B, nx).
 *
 * Bad arguments (NULL buffers, chain_nx not dividing N or E != 2N with
 * chain_nx > 0, layers > 8, non-positive sizes, a workspace_bytes too small)
 * return HF_EINVAL before any device call; the size queries return -1.
 */
int64_t hf_pure_gnn_tape_bytes(int in_dim, int hidden, int layers, int64_t N, int64_t E);
int64_t hf_pure_gnn_backward_workspace_bytes(int in_dim, int hidden, int layers, int64_t N, int64_t E);
int hf_pure_gnn_forward_train(const float *dev_params, int in_dim, int hidden, int layers,
                              const float *dev_node_features, int64_t N, const int64_t *dev_edge_index,
                              int64_t E, int chain_nx, float *dev_delta, void *dev_tape, void *stream);
int hf_pure_gnn_backward(const float *dev_params, int in_dim, int hidden, int layers,
                         const float *dev_node_features, int64_t N, const int64_t *dev_edge_index,
                         int64_t E, int chain_nx, const void *dev_tape, const float *dev_grad_delta,
                         float *dev_grad_params, float *dev_grad_node_features /* or NULL */,
                         void *dev_workspace, void *stream);
int64_t hf_state_mse_workspace_bytes(int B, int nx);
int hf_state_mse(const float *dev_delta, const float *dev_state_t, const float *dev_state_next,
                 int B, int nx, float *dev_loss, float *dev_grad_delta, void *dev_workspace,
                 int64_t workspace_bytes, void *stream);

/*
 * Unrolled training of PureGNN: the model differentiated through K steps of
 * its own rollout.  Replaces: scripts/evaluation/evaluate_multi_ic.py:53-64
 * under autograd -- the torch ops a user would put around PureGNN's autograd
 * Function to train through state <- state + PureGNN([n, u, E, x]) (permute,
 * reshape, cat, add, the weighted MSE against the classical trajectory and
 * their autograd mirrors, about 20 small launches per unrolled step on tensors
 * in two layouts) -- by one launch per forward step and one per backward step
 * around hf_pure_gnn_forward_train / hf_pure_gnn_backward.  The reference
 * trains PureGNN one step at a time (hf_state_mse above).
 *
 * Step k maps s_k [B][3][nx] to s_{k+1} = s_k + delta_k^T with delta_k =
 * PureGNN([n, u, E, x]) [B*nx][3], and the loss is hf_unroll_update's:
 * L = (1/K) sum_k mean_{b,ch,i} w_ch (s_k - s*_k)^2, k = 1..K.
 *
 * hf_pure_unroll_update (replaces evaluate_multi_ic.py:53-64 under autograd,
 * forward): dev_state_next[b][ch][i] = dev_state[b][ch][i] +
 * dev_delta[b*nx+i][ch], one float32 add per value (bit-equal to the torch
 * expression), and, when not NULL, dev_node_features_next [B*nx][4] =
 * [n', u', E', x_i], exact copies: the next step's PureGNN input.  With
 * dev_target [B][3][nx] (else NULL: no loss, and dev_loss, weights and the
 * workspace are not used) it also writes dev_loss[0] = loss_scale *
 * sum_{b,ch,i} weights[ch] (s' - target)^2 (weights: 3 HOST floats; loss_scale
 * = 1 / (K 3 B nx) gives the step's term of L): float64 partials per workgroup
 * through dev_workspace (hf_pure_unroll_workspace_bytes(B, nx); the call zeroes
 * its arrival counter itself with a memset node), summed in workgroup order by
 * the last workgroup to arrive, no float atomics: two calls give the same bits.
 *
 * hf_pure_unroll_adjoint (replaces evaluate_multi_ic.py:53-64 under autograd,
 * backward): with seed = 2 weights[ch] loss_scale (dev_state_next - dev_target)
 * [b][ch][i],
 *   dev_grad_delta[b*nx+i][ch] = (seed + dev_grad_delta_next[b*nx+i][ch])
 *                                + dev_grad_nf_next[b*nx+i][ch].
 * dev_grad_delta_next [B*nx][3] is what this call wrote for step k+1 and
 * dev_grad_nf_next [B*nx][4] hf_pure_gnn_backward's dL/dnode_features of step
 * k+1 (column 3, dL/dx, is not used); both NULL at the last step, and at every
 * step for the pushforward form, which cuts the state gradient between steps.
 * A NULL term is left out of the sum, not added as zero.  The residual update
 * is the identity in the state, so dL/ds_{k+1} transposed IS dL/ddelta_k: no
 * separate direct part.  Every value is written by one thread in that order.
 *
 * Kernels: one 256-thread workgroup per tile of 1024 cells of an IC, the
 * (cell, channel) <-> (channel, cell) transposition staged through LDS so both
 * layouts move lane after lane; node features as 16-byte stores.  Any nx >= 1
 * and B >= 1 with B * ceil(nx / 1024) < 2^31.  Before any device call: NULL
 * required pointers, B < 1, nx < 1, that product too large, dev_state_next ==
 * dev_state, a target without dev_loss, weights or workspace, or a
 * workspace_bytes too small return HF_EINVAL (hf_pure_unroll_workspace_bytes:
 * -1).
 */
int64_t hf_pure_unroll_workspace_bytes(int B, int nx);
int hf_pure_unroll_update(const float *dev_delta, const float *dev_state, const float *dev_x, int B, int nx,
                          float *dev_state_next, float *dev_node_features_next /* or NULL */,
                          const float *dev_target /* or NULL */, const float *weights, float loss_scale,
                          float *dev_loss, void *dev_workspace, int64_t workspace_bytes, void *stream);
int hf_pure_unroll_adjoint(const float *dev_state_next, const float *dev_target, const float *weights,
                           float loss_scale, const float *dev_grad_delta_next /* or NULL */,
                           const float *dev_grad_nf_next /* or NULL */, int B, int nx, float *dev_grad_delta,
                           void *stream);

int64_t hf_pinn_param_count(int dim, int hidden, int layers);
int64_t hf_pinn_workspace_bytes(int dim, int hidden, int64_t B);
int hf_pinn_forward(const float *dev_params, int dim, int hidden, int layers, const float *dev_state,
                    float *dev_out, int64_t B, void *dev_workspace, void *stream);
int hf_pinn_run(const float *dev_params, int dim, int hidden, int layers, const float *dev_state0,
                float *dev_final, int64_t B, int T, float *dev_traj, void *dev_workspace, void *stream);

/*
 * PINN training (scripts/training/train_pinn.py), in the style of the PureGNN
 * training entry points above.  dev_params and dev_grad_params are flat
 * float32 device buffers of hf_pinn_param_count values in state-dict order;
 * 2 <= layers <= 8 (as hf_pinn_run), B >= 1, dim = 3 nx.
 *
 * hf_pinn_forward_train (train_pinn.py:51-61 under autograd) writes dev_out
 * [B][dim] = state + net(state) and a tape (hf_pinn_tape_bytes: the layers - 1
 * tanh activations) that hf_pinn_backward consumes.  Its values are
 * hf_pinn_forward's to rounding, not bit for bit (that one-launch kernel sums
 * k in a permuted order).
 *
 * hf_pinn_backward (loss.backward() of :178 through :51-61) reads dev_grad_out
 * = dL/dout [B][dim] and writes dL/dparams (overwriting, the layout of
 * dev_params) and, when dev_grad_state is not NULL, dL/dstate = grad_out +
 * grad_out dnet/dstate; workspace hf_pinn_backward_workspace_bytes.
 * dev_params must be unchanged between the forward that wrote the tape and
 * the backward (the backward multiplies by the weights the forward used), so
 * the optimizer step comes after it.
 *
 * hf_pinn_loss (:64-111 and :163-175) is one launch.  With s = dev_state_t, s*
 * = dev_state_next, p = dev_pred (all [B][3][nx]), d = p - s*, (n, u, E) the
 * rows of s, periodic indices, N3 = 3 B nx, N1 = B nx:
 *   r_c[i] = (p_n[i] - n[i])/dt + (n[i+1]u[i+1] - n[i-1]u[i-1])/(2dx)
 *   r_m[i] = (p_u[i] - u[i])/dt + u[i](u[i+1] - u[i-1])/(2dx) + E[i]
 *            - nu (u[i+1] - 2u[i] + u[i-1])/dx^2
 *   r_p[i] = p_E[i] - X[i],  X[0] = 0,  X[i] = -(P p_n)[i] for i >= 1
 *   dev_losses = (w_d data + w_c cont + w_m mom + w_p pois, data = sum d^2/N3,
 *                 cont = sum r_c^2/N1, mom = sum r_m^2/N1, pois = sum r_p^2/N1)
 * with weights = (w_d, w_c, w_m, w_p), 4 HOST floats, and P the spectral
 * Poisson operator: the circulant whose first column is dev_plan[0..nx) of
 * hf_poisson_coeffs(nx, nx dx).  X is the reference trainer's
 * solve_poisson_torch (:64-75), not the solver's field: the opposite sign, and
 * cell 0 set to zero.  dev_grad_pred [B][3][nx] = dL/dp; the Poisson term is
 * not detached (P^T = -P, r~ = r_p with r~[0] = 0):
 *   dL/dp_n = 2 w_d d_n/N3 + 2 w_c r_c/(dt N1) - (2 w_p/N1) (P r~)
 *   dL/dp_u = 2 w_d d_u/N3 + 2 w_m r_m/(dt N1)
 *   dL/dp_E = 2 w_d d_E/N3 + 2 w_p r_p/N1            (cell 0 included)
 * One workgroup per IC with the circulant column, p_n and r~ in LDS
 * (nx <= 6144; larger: HF_EUNSUPPORTED); residuals and sums in float64, the
 * per-IC partial sums added in a fixed order by the last workgroup to arrive
 * (its counter is zeroed by the call), no float atomics.  dev_workspace:
 * hf_pinn_loss_workspace_bytes(B, nx).
 *
 * Shapes with dim and hidden multiples of 32 run on the f32 MFMA GEMMs of
 * csrc/tgemm.h (layers launches forward, layers + 3 backward), every other
 * shape on the generic GEMMs.  Every sum runs in a fixed order (split-K
 * weight gradients reduced in split order): two calls on the same inputs give
 * the same bits.
 *
 * Bad arguments (NULL required pointers, B < 1, nx < 1, layers outside 2..8,
 * non-positive dims, dev_out == dev_state, a workspace_bytes too small) return
 * HF_EINVAL before any device call; the size queries return -1.
 */
int64_t hf_pinn_tape_bytes(int dim, int hidden, int layers, int64_t B);
int64_t hf_pinn_backward_workspace_bytes(int dim, int hidden, int layers, int64_t B);
int64_t hf_pinn_loss_workspace_bytes(int B, int nx);
int hf_pinn_forward_train(const float *dev_params, int dim, int hidden, int layers, const float *dev_state,
                          int64_t B, float *dev_out, void *dev_tape, void *stream);
int hf_pinn_backward(const float *dev_params, int dim, int hidden, int layers, const float *dev_state, int64_t B,
                     const void *dev_tape, const float *dev_grad_out, float *dev_grad_params,
                     float *dev_grad_state /* or NULL */, void *dev_workspace, int64_t workspace_bytes,
                     void *stream);
int hf_pinn_loss(const float *dev_pred, const float *dev_state_t, const float *dev_state_next, int B, int nx,
                 double dt, double dx, double nu, const float *weights /* 4 host floats */,
                 const double *dev_plan, float *dev_losses /* [5] */, float *dev_grad_pred,
                 void *dev_workspace, int64_t workspace_bytes, void *stream);

/*
 * Unrolled training of PINN: the network differentiated through K steps of its
 * own rollout s^_k = s^_{k-1} + net(s^_{k-1}), s^_0 = s*_0
 * (scripts/evaluation/evaluate_multi_ic.py:70-83), around
 * hf_pinn_forward_train / hf_pinn_backward.  For a window of targets s*_0..s*_K
 *   L = (1/K) sum_{k=1..K} [ mean_{b,ch,i} w_ch (s^_k - s*_k)^2
 *         + l_c mean_{b,i} r_c^2 + l_m mean_{b,i} r_m^2 + l_p mean_{b,i} r_p^2 ]
 * with r_c, r_m, r_p hf_pinn_loss's residuals at p = s^_k, (n, u, E) = s^_{k-1}
 * (the model's own previous state, so the residuals carry a gradient into it,
 * which hf_pinn_loss does not have).  l = (0, 0, 0) is hf_unroll_update's and
 * hf_pure_unroll_update's L; K = 1, w = (1, 1, 1), l = (0.1, 0.1, 0.01) is
 * hf_pinn_loss with the reference's weights.
 *
 * hf_pinn_unroll_loss, step k's term: p = dev_pred = s^_k, dev_state =
 * s^_{k-1}, dev_target = s*_k, all [B][3][nx].  dev_losses[0..4] = (total,
 * data, cont, mom, pois): data = loss_scale sum w_ch (p - s*)^2, cont =
 * phys_scale l_c sum r_c^2, mom = phys_scale l_m sum r_m^2, pois = phys_scale
 * l_p sum r_p^2, total their sum; loss_scale = 1/(K 3 B nx) and phys_scale =
 * 1/(K B nx) give the step's term of L.  weights = w, 3 HOST floats; phys = (l_c,
 * l_m, l_p), 3 HOST floats, or NULL: entries 2..4 are 0, dev_state and dev_plan
 * are not read and no O(nx^2) Poisson work is done (nor is it with l_p = 0).
 * The data term is hf_pure_unroll_update's sum term for term (the float32
 * difference squared in float64): with phys NULL and nx <= 1024 the total equals
 * that call's loss bit for bit; beyond 1024 cells that kernel cuts its partials
 * per tile, this one per IC.
 *
 * hf_pinn_unroll_adjoint, step k's incoming gradient for hf_pinn_backward, three
 * parts, a NULL term left out of the sum, not added as zero:
 *   dev_grad_out = d term_k / d p              (p = dev_pred, state slot dev_state)
 *                + d term_{k+1} / d (state slot) (with phys and dev_pred_next =
 *                    s^_{k+1}: the residuals of step k+1 at p' = dev_pred_next,
 *                    (n, u, E) = dev_pred)
 *                + dev_grad_state_next         (hf_pinn_backward's dL/dstate of step k+1)
 * Part 1 is hf_pinn_loss's dL/dp with 2 w_ch loss_scale (p - s*) per channel
 * and the factors 2 phys_scale l (the -(P r~) term on the n row included).
 * Part 2, with q_c = 2 phys_scale l_c r_c and q_m = 2 phys_scale l_m r_m of step
 * k+1, periodic indices, (n, u, E) = dev_pred:
 *   d/dn[j] = -q_c[j]/dt + u[j](q_c[j-1] - q_c[j+1])/(2dx)
 *   d/du[j] = n[j](q_c[j-1] - q_c[j+1])/(2dx)
 *           + q_m[j](-1/dt + (u[j+1] - u[j-1])/(2dx) + 2nu/dx^2)
 *           + q_m[j-1](u[j-1]/(2dx) - nu/dx^2) + q_m[j+1](-u[j+1]/(2dx) - nu/dx^2)
 *   d/dE[j] = q_m[j]
 * (r_p does not depend on the state slot; the neighbour terms stay separate
 * terms where indices coincide, nx = 1, 2).  The last step passes NULL for
 * dev_pred_next and dev_grad_state_next, the pushforward form at every step.
 *
 * Kernels: one 256-thread workgroup per IC; the circulant column, p_n - 1, r~
 * and q_c, q_m in LDS (16 nx bytes; nx <= 6144, larger: HF_EUNSUPPORTED);
 * spectral operator only (dev_plan[0..nx) of hf_poisson_coeffs(nx, nx dx));
 * residuals and sums in float64; per-IC float64 partials through dev_workspace
 * (hf_pinn_unroll_workspace_bytes(B, nx); the call zeroes its arrival counter
 * itself), summed in IC order by the last workgroup to arrive; no float atomics;
 * every output value is written by one thread in a fixed order: two calls give
 * the same bits.  Before any device call a NULL required pointer, B < 1, nx < 1,
 * phys without dev_plan or dev_state (or with dt <= 0 or dx <= 0), a
 * workspace_bytes too small, or dev_grad_out equal to an input return HF_EINVAL
 * (the size query: -1).
 */
int64_t hf_pinn_unroll_workspace_bytes(int B, int nx);
int hf_pinn_unroll_loss(const float *dev_pred, const float *dev_state, const float *dev_target, int B, int nx,
                        const float *weights /* 3 host */, float loss_scale,
                        const float *phys /* 3 host: l_c, l_m, l_p; or NULL */, float phys_scale, double dt, double dx,
                        double nu, const double *dev_plan /* required iff phys */, float *dev_losses /* [5] */,
                        void *dev_workspace, int64_t workspace_bytes, void *stream);
int hf_pinn_unroll_adjoint(const float *dev_pred, const float *dev_state, const float *dev_target,
                           const float *dev_pred_next /* or NULL */, const float *dev_grad_state_next /* or NULL */,
                           int B, int nx, const float *weights, float loss_scale, const float *phys, float phys_scale,
                           double dt, double dx, double nu, const double *dev_plan, float *dev_grad_out, void *stream);

/*
 * Unrolled training: energy and charge terms with live gradients, for all
 * three rollout trainers.  Replaces: nothing the reference trains on -- its
 * charge, energy_one and energy_multi terms carry no gradient (see
 * hf_ablation_loss_ex above); under a K-step loss they do, because u_{k+1}
 * depends on the parameters through E_k and E_{k+1} through n_{k+1}, and for
 * PureGNN and PINN, which conserve nothing by construction, so does charge.
 *
 * With e(s)_b = 0.5 (sum_i u_i^2 + sum_i E_i^2) / nx and q(s)_b = (sum_i n_i) /
 * nx (HF_NUM_METRICS [0] and [1]), a reference (eref_b, qref_b) per IC of the
 * step, r_e = e(s^_k)_b - eref_b and r_q = q(s^_k)_b - qref_b, a step adds
 *   cons_scale sum_b [ lam_e r_e^2 + lam_q r_q^2 ]      (cons_scale = 1 / (K B))
 * to its term of L.  The sums and the residuals are float64 from the float32
 * state, the squares taken in float64; e is never rounded to float32.  Its
 * gradient with respect to s^_k is rank one per IC: d/du_i = ce_b u_i, d/dE_i =
 * ce_b E_i, d/dn_i = cq_b with ce_b = 2 lam_e cons_scale r_e / nx and cq_b = 2
 * lam_q cons_scale r_q / nx, which the forward call leaves in dev_cons_coef
 * [B][2] = (ce, cq), computed in float64 and rounded to float32 once.
 *
 * hf_state_moments: dev_moments [rows][2] = (e, q) of dev_states [rows][3][nx],
 * float64, one wave per row in a fixed order (a lane's cells ascending, the
 * lanes in a fixed tree): two calls give the same bits.  Any nx >= 1.  One call
 * on a whole window [K+1][B] gives every step's reference as a pointer into
 * its output.
 *
 * hf_unroll_update_ex, hf_pure_unroll_update_ex, hf_pinn_unroll_loss_ex: the
 * plain calls' arguments, with the loss row dev_losses in place of the single
 * float -- (total, state, energy, charge) for the two GNNs, (total, data, cont,
 * mom, pois, energy, charge) for PINN -- and cons (2 HOST floats lam_e, lam_q,
 * or NULL), cons_scale, dev_cons_ref [B][2] float64 and dev_cons_coef [B][2].
 * The per-IC sums of u^2, E^2 and n ride the reduction the kernel makes for its
 * loss partial, float64 per workgroup through the workspace
 * (hf_*_workspace_bytes_ex(B, nx)), no float atomics.  Whoever holds an IC's
 * complete sums writes its coefficients: the IC's own workgroup (or wave, at the
 * FFT sizes) in the hybrid and PINN kernels; in PureGNN's kernel, which cuts an
 * IC into 1024-cell tiles, the last workgroup to arrive, adding the tiles in
 * tile order.  The last arriver adds the ICs' values in IC order: two calls
 * give the same bits.  State, node features and the state (data, residual)
 * values are the plain calls' bit for bit.  With cons == NULL (then
 * dev_cons_ref and dev_cons_coef must be NULL, and the plain workspace size
 * is enough) total equals the plain call's loss and energy = charge = 0.  cons
 * needs dev_target.
 *
 * hf_unroll_adjoint_ex, hf_pure_unroll_adjoint_ex, hf_pinn_unroll_adjoint_ex:
 * the plain calls' arguments and dev_cons_coef ([B][2] or NULL: the plain
 * call's bits).  The seed of s^_{k+1} gains (cq_b, ce_b u, ce_b E) on its three
 * channels: one float32 product (none for cq) and one add per value, and the
 * order of the sum is
 *   ((2 w_ch loss_scale (s^ - s*) + new part) + ...the plain call's further terms in their order)
 * -- hybrid: then grad_nf_next, then direct_next; PureGNN: then
 * grad_delta_next, then grad_nf_next; PINN (whose sum is float64, the product
 * float32): then the residual terms, part 2 and the carry.  The hybrid adjoint
 * does not add cq: the finite-volume update conserves sum n identically (the
 * face fluxes telescope), so the charge term's parameter gradient is
 * identically 0 there and adding it would only inject rounding noise; the
 * charge value is still reported.
 *
 * HF_EINVAL before any device call: cons without dev_target, dev_cons_ref,
 * dev_cons_coef or a workspace; dev_cons_ref or dev_cons_coef without cons; a
 * lam that is negative or NaN; a workspace smaller than the _ex query with
 * cons; and everything the plain calls refuse (nx limits unchanged).  The size
 * queries return -1 as the plain ones do.
 */
int hf_state_moments(const float *dev_states, int64_t rows, int nx, double *dev_moments, void *stream);
int64_t hf_unroll_workspace_bytes_ex(int B, int nx);
int hf_unroll_update_ex(const float *dev_flux_edge, const float *dev_state, const float *dev_x, const double *dev_plan,
                        int poisson_mode, int B, int nx, float c, float dt, float *dev_state_next,
                        float *dev_node_features_next /* or NULL */, const float *dev_target /* or NULL */,
                        const float *weights, float loss_scale, float *dev_losses /* [4] */, void *dev_workspace,
                        int64_t workspace_bytes, const float *cons /* 2 host: lam_e, lam_q; or NULL */,
                        float cons_scale, const double *dev_cons_ref, float *dev_cons_coef, void *stream);
int hf_unroll_adjoint_ex(const float *dev_state, const float *dev_state_next, const float *dev_target,
                         const float *weights, float loss_scale, const float *dev_direct_next /* or NULL */,
                         const float *dev_grad_nf_next /* or NULL */, const double *dev_plan, int poisson_mode, int B,
                         int nx, float c, float dt, float *dev_grad_flux_edge, float *dev_direct /* or NULL */,
                         const float *dev_cons_coef /* or NULL */, void *stream);
int64_t hf_pure_unroll_workspace_bytes_ex(int B, int nx);
int hf_pure_unroll_update_ex(const float *dev_delta, const float *dev_state, const float *dev_x, int B, int nx,
                             float *dev_state_next, float *dev_node_features_next /* or NULL */,
                             const float *dev_target /* or NULL */, const float *weights, float loss_scale,
                             float *dev_losses /* [4] */, void *dev_workspace, int64_t workspace_bytes,
                             const float *cons /* 2 host; or NULL */, float cons_scale, const double *dev_cons_ref,
                             float *dev_cons_coef, void *stream);
int hf_pure_unroll_adjoint_ex(const float *dev_state_next, const float *dev_target, const float *weights,
                              float loss_scale, const float *dev_grad_delta_next /* or NULL */,
                              const float *dev_grad_nf_next /* or NULL */, int B, int nx, float *dev_grad_delta,
                              const float *dev_cons_coef /* or NULL */, void *stream);
int64_t hf_pinn_unroll_workspace_bytes_ex(int B, int nx);
int hf_pinn_unroll_loss_ex(const float *dev_pred, const float *dev_state, const float *dev_target, int B, int nx,
                           const float *weights /* 3 host */, float loss_scale,
                           const float *phys /* 3 host: l_c, l_m, l_p; or NULL */, float phys_scale, double dt,
                           double dx, double nu, const double *dev_plan /* required iff phys */,
                           float *dev_losses /* [7] */, void *dev_workspace, int64_t workspace_bytes,
                           const float *cons /* 2 host; or NULL */, float cons_scale, const double *dev_cons_ref,
                           float *dev_cons_coef, void *stream);
int hf_pinn_unroll_adjoint_ex(const float *dev_pred, const float *dev_state, const float *dev_target,
                              const float *dev_pred_next /* or NULL */, const float *dev_grad_state_next /* or NULL */,
                              int B, int nx, const float *weights, float loss_scale, const float *phys,
                              float phys_scale, double dt, double dx, double nu, const double *dev_plan,
                              float *dev_grad_out, const float *dev_cons_coef /* or NULL */, void *stream);

/*
 * Host helper (no device work): the Poisson "plan" for nx cells, length
 * hf_poisson_plan_len(nx) doubles.  plan[0..nx) is the first column c of the
 * real circulant matrix equal to the reference's spectral Poisson operator
 * E = Re(ifft(1j*fft(n-1)/k)), k=0 mode zeroed (src/baseline_solver.py:26,59-68):
 * E[i] = sum_j c[(i-j) mod nx] * (n[j]-1), computed in float64.  For power-of-two
 * nx in [256, 2048] the kernels apply the operator by float64 FFT instead and
 * the plan continues with the twiddles exp(-2 pi i m/nx), m < nx/2, as (re, im)
 * pairs, then 1/k_q (0 for q = 0 and, for even nx, q = nx/2: that term is imaginary for real rho, dropped by the reference's Re()).  Every dev_c argument below is a device copy
 * of this plan.
 */
int hf_poisson_plan_len(int nx);
int hf_poisson_coeffs(int nx, double length, double *host_c);

/* Replaces: BaselineSolver.solve_poisson (src/baseline_solver.py:59-68), batched.
 * dev_n, dev_E: [B][nx] float32 (row stride ld_n / ld_E floats);
 * dev_c: device copy of hf_poisson_coeffs. */
int hf_poisson(const float *dev_n, int ld_n, float *dev_E, int ld_E,
               const double *dev_c, int B, int nx, void *stream);

/*
 * Poisson modes.  Every entry point without a mode argument, and every *_ex
 * call given HF_POISSON_SPECTRAL, applies the reference's spectral operator
 * (src/baseline_solver.py:59-68) with the plan of hf_poisson_coeffs: the
 * parity mode and the default.
 *
 * HF_POISSON_TRIDIAG is an OPT-IN mode that is NOT the reference's operator
 * (no parity with the reference is claimed for it): the cyclic-reduction
 * tridiagonal solve the north star names, of the same equation dE/dx =
 * -(rho - mean rho), rho = n - 1, in second-order potential form on the
 * periodic grid:
 *   (phi[i-1] - 2 phi[i] + phi[i+1]) / dx^2 = rho[i] - mean(rho),
 *   E[i] = -(phi[i+1] - phi[i-1]) / (2 dx),
 * solved in float64 by one wave per IC (or IC pair) with phi[0] = 0 (E does not
 * depend on the gauge) and rounded to float32 once.  It differs from the
 * spectral E by ~1e-3 at nx = 64 (the symbol (dx/2) cot(k dx/2) vs 1/k).
 * Fused into the same kernels as the spectral solve (the persistent rollouts
 * at nx <= 64, the FV kernels at every other nx); nx <= 16384.  The training
 * loss (hf_ablation_loss) always uses the spectral operator.
 */
#define HF_POISSON_SPECTRAL 0
#define HF_POISSON_TRIDIAG 1
/* Length in doubles of the plan of `mode` for nx cells (-1: unsupported):
 * hf_poisson_plan_len(nx) for SPECTRAL, 1 for TRIDIAG (plan[0] = dx/2). */
int hf_poisson_plan_size(int mode, int nx);
/* Host helper (no device work): the plan of `mode` (SPECTRAL: hf_poisson_coeffs). */
int hf_poisson_plan(int mode, int nx, double length, double *host_plan);
/* hf_poisson with a Poisson mode; dev_plan is a device copy of hf_poisson_plan(mode, ...). */
int hf_poisson_ex(const float *dev_n, int ld_n, float *dev_E, int ld_E, const double *dev_plan,
                  int poisson_mode, int B, int nx, void *stream);

/*
 * Initial conditions on the device.
 * Replaces: the per-seed host loop over BaselineSolver.initial_condition
 * (src/baseline_solver.py:29-51): np.random.RandomState(seed), 3-5 sine modes
 * on n, two cosine modes and 0.05 * randn(nx) on u.  The kernel consumes the
 * 32-bit words of MT19937 exactly as numpy's legacy RandomState does
 * (init_genrand seeding; randint by masked rejection, one word per try; rand
 * from two words; the polar gauss, four words per attempt) and evaluates
 *   n[i] = 1 + sum_m f32(amp_m) * f32(sin(km_m x[i] + ph_m))
 *   u[i] = sum_m f32(amp_m) * f32(cos(km_m x[i] + ph_m)) + f32(0.05) * f32(gauss[i])
 * with the argument and sin / cos in float64 and every product and sum in
 * float32, in the reference's order.  One wave per seed.  Rows n and u of
 * dev_state [B][3][nx] are written; row E is left alone (hf_poisson fills it).
 *
 * dev_seeds: [B] int64, each in [0, 2^32) (numpy's integer-seed path); dev_x:
 * [nx] float64 cell centres.  numpy's rejection loops have no bound; here each
 * randint gives up after 64 tries and the gauss after 2 nx + 256 attempts
 * (probability < 4^-64 with a correct generator), and an IC whose draws gave
 * up, or whose seed is out of range, gets NaN in every cell of n and u.
 *
 * dev_table (or NULL): [B][HF_IC_TABLE_LEN] float64, per IC
 *   [0]          number of n modes (3..5; -1: the draws gave up)
 *   [1 + 3 s..]  (km, amp, ph) of slot s: s = 0..4 the n modes (unused: 0),
 *                s = 5, 6 the two u modes
 *   [22]         32-bit words consumed
 * None of it passes through sin, cos or log, so it equals numpy's exactly.
 *
 * hf_ic_draws_host: host only (no device work), the same draw code for one
 * seed: host_table [HF_IC_TABLE_LEN] as above and host_gauss [nx] float64, the
 * values of randn(nx) after the mode draws.
 */
#define HF_IC_TABLE_LEN 23
int hf_initial_conditions(const int64_t *dev_seeds, int B, int nx, const double *dev_x, float *dev_state,
                          double *dev_table /* or NULL */, void *stream);
int hf_ic_draws_host(int64_t seed, int nx, double *host_table, double *host_gauss);

/*
 * Training noise on the device: a seeded Gaussian perturbation of a batch of
 * states, for training on perturbed start states against clean targets.
 *
 * Draws.  For sample b, g = np.random.RandomState(seed_b).standard_normal(3 nx):
 * the legacy polar method from word 0 of a freshly seeded MT19937 stream (four
 * words per attempt, an accepted attempt yields f x2 then f x1), the draw code
 * of hf_initial_conditions without the mode draws, one wave per sample.  The
 * blocks are g_n = g[0:nx], g_u = g[nx:2nx], g_E = g[2nx:3nx].  All 3 nx values
 * are always drawn, whatever sigma and flags say: the stream does not depend on
 * the options.
 *
 * Arithmetic, per channel ch with s = sigma[ch] (3 HOST floats: n, u, E):
 *   out[ch][i] = in[ch][i] + (float)s * (float)d[i]
 * one float32 product, then one float32 add, no FMA.  d = g_ch in float64.
 * With HF_NOISE_ZERO_MEAN, and for ch = n only, d[i] = g_n[i] - m with
 * m = (float64 sum of g_n) / nx, so the perturbation leaves the charge sum n
 * alone up to float32 rounding.  The sum is taken in one fixed order: lane l of
 * the wave adds its cells l, l + 64, l + 128, ... in ascending order from 0.0,
 * then the 64 lane sums are combined in a fixed tree (v[l] += v[l ^ o] for o =
 * 32, 16, 8, 4, 2, 1): two calls give the same bits.  sigma[ch] == 0: the row
 * is copied bit for bit (no add happens: -0.0 and NaN payloads survive).
 *
 * Poisson.  With dev_plan not NULL sigma[2] must be 0, and row E of the output
 * is hf_poisson_ex(poisson_mode) of the perturbed n row, bit for bit (the
 * existing launcher on the row with stride 3 nx): the perturbed state is a
 * consistent solver state.  Without a plan E follows the rule above.  (At the
 * FFT sizes, power-of-two nx in [256, 2048], that launcher transforms samples
 * 2k and 2k+1 as one complex row, so a sample's float64 path depends on its
 * pair partner.  E' has been bit-equal alone and in any batch wherever tested,
 * because the rounding to float32 absorbs the difference; that is observed, not
 * true by construction, and is hf_poisson_ex's property, not this call's.)
 *
 * dev_state_in, dev_state_out: [B][3][nx]; dev_state_out may be dev_state_in
 * (any other overlap is not allowed).  dev_node_features (or NULL; needs dev_x
 * [nx] float32): [B nx][4] = [n', u', E', x], exact copies, written after E' is
 * final.  dev_noise (or NULL): [B][3][nx], the float32 values (float)s *
 * (float)d[i] that were added; 0 on a copied row and on a recomputed E row.
 *
 * A seed outside [0, 2^32), or draws that give up (after 2 (3 nx) + 256
 * attempts, as in hf_initial_conditions), make rows n, u, E of that sample NaN
 * (dev_noise and its node features too) and leave the other samples intact.
 * With a plan the failed sample enters the Poisson solve with n = 1 (a NaN row
 * would reach its pair partner at the FFT sizes); the draws mark it by filling
 * its u row with the quiet NaN 0x7fd0bad5, and the last launch turns every
 * sample whose u row holds that word in every cell NaN.  (An input whose u row
 * is that word throughout, under a plan, is therefore treated as failed.)
 *
 * At most three launches on `stream` (the draws; the Poisson solve; the failed
 * samples' NaN and the node features), no allocation, no host synchronisation:
 * capturable.
 *
 * HF_EINVAL before any device call: a NULL dev_seeds, sigma, dev_state_in or
 * dev_state_out (with B > 0); B < 0 or nx < 1; a negative or NaN sigma; unknown
 * flags; sigma[2] != 0 or an unknown Poisson mode with a plan;
 * dev_node_features without dev_x.  HF_EUNSUPPORTED: nx > 2^24; nx > 6144 with
 * HF_NOISE_ZERO_MEAN (g_n is held in LDS for the second pass); a Poisson mode
 * that does not take this nx.  B = 0 is HF_OK without a launch.
 *
 * hf_gauss_host: host only (no device work), the same draw code:
 * host_gauss[0..count) = RandomState(seed).standard_normal(count).  -1
 * (HF_EINVAL) for a seed outside [0, 2^32), count < 0 or a NULL host_gauss with
 * count > 0.
 */
#define HF_NOISE_ZERO_MEAN 1   /* remove the mean of the n noise: charge is kept */
int hf_state_noise(const int64_t *dev_seeds, int B, int nx, const float *sigma /* 3 HOST floats: n, u, E */,
                   int flags, const float *dev_state_in, float *dev_state_out /* may be dev_state_in */,
                   const double *dev_plan /* or NULL */, int poisson_mode,
                   const float *dev_x /* or NULL */, float *dev_node_features /* or NULL */,
                   float *dev_noise /* or NULL */, void *stream);
int hf_gauss_host(int64_t seed, int64_t count, double *host_gauss);   /* host only, no device work */

/*
 * Scratch of the generic (non-fused) sequencing.  hf_step, hf_run and
 * hf_run_compare take (dev_workspace, workspace_bytes): a device buffer of at
 * least hf_workspace_need(model, op, B, nx, T, flags) bytes (or the upper
 * bound hf_run_workspace_bytes(op, B, nx, T)) that the call may use as
 * scratch until the work it enqueued has run; the caller keeps it alive and
 * unshared until then.  dev_workspace == NULL makes the call allocate its
 * scratch stream-ordered (hipMallocAsync / hipFreeAsync on `stream`).  The
 * fused paths (nx in {16,32,48,64} with a model) use no scratch.
 */
#define HF_OP_STEP 0
#define HF_OP_RUN 1
#define HF_OP_COMPARE 2
/* An upper bound over every model, nx path and output choice of `op`. */
int64_t hf_run_workspace_bytes(int op, int B, int nx, int T);
/* The exact scratch the call will carve for this model (NULL = classical;
 * HF_OP_COMPARE needs a model), nx path and outputs: flags HF_WS_TRAJ when the
 * call is given dev_traj (hf_run), HF_WS_FLUX_FACE when given dev_flux_face
 * (hf_step).  0 on every path that needs no scratch (the fused rollouts, the
 * one-launch classical rollouts); -1 on bad arguments.  A dev_workspace of at
 * least this many bytes is accepted by the call; a smaller one is HF_EINVAL. */
#define HF_WS_TRAJ 1
#define HF_WS_FLUX_FACE 2
int64_t hf_workspace_need(hf_model_t model, int op, int B, int nx, int T, int flags);

/*
 * One timestep for B ICs (state_in -> state_out, may not alias).
 * model != NULL: HybridSolver.step (src/hybrid_solver.py:34-64):
 *   GNN flux -> symmetrise -> FV continuity -> Burgers u (no viscosity) -> Poisson.
 * model == NULL: BaselineSolver.step (src/baseline_solver.py:80-101):
 *   F=n*u -> FV continuity -> Burgers u + dt*(E + nu*lap u) -> Poisson.
 * Scalars are the reference's Python floats rounded to float32 on the host:
 *   c = f32(dt/dx), dt = f32(dt), nu = f32(nu), dx2 = f32(dx*dx).
 * dev_x [nx]: float32 cell centres (node feature x); dev_c: Poisson coeffs.
 * dev_flux_face [B][nx] (may be NULL): the F used this step (F_n classically).
 * dev_metrics [B][HF_NUM_METRICS] (may be NULL) for state_out.
 * Any nx >= 1: nx <= 6144 keeps the chain in LDS; larger nx (not an FFT size)
 * runs the update and a tiled Poisson sum over global memory, same values.
 */
int hf_step(hf_model_t model, const float *dev_state_in, float *dev_state_out,
            const float *dev_x, const double *dev_c, int B, int nx,
            float c, float dt, float nu, float dx2,
            float *dev_flux_face, float *dev_metrics,
            void *dev_workspace, int64_t workspace_bytes, void *stream);
/* hf_step with a Poisson mode (dev_plan: hf_poisson_plan(poisson_mode, ...));
 * hf_step == hf_step_ex(..., dev_c, HF_POISSON_SPECTRAL, ...). */
int hf_step_ex(hf_model_t model, const float *dev_state_in, float *dev_state_out,
               const float *dev_x, const double *dev_plan, int poisson_mode, int B, int nx,
               float c, float dt, float nu, float dx2,
               float *dev_flux_face, float *dev_metrics,
               void *dev_workspace, int64_t workspace_bytes, void *stream);

/*
 * T-step rollout (HybridSolver.run src/hybrid_solver.py:66-73 when model !=
 * NULL, BaselineSolver.run src/baseline_solver.py:103-118 when NULL), batched.
 * dev_state0 [B][3][nx] -> dev_state_final [B][3][nx]; the two may alias
 * (the same buffer holds the initial and, after the call, the final states).
 * dev_traj [B][T+1][3][nx] (may be NULL) receives every state incl. t=0.
 * dev_flux_traj [B][T][nx] (may be NULL) receives the face flux of each step
 *   (the classical run's `fluxes`).
 * dev_metrics [B][T+1][HF_NUM_METRICS] (may be NULL).
 * For nx in {16,32,48,64} with model != NULL the whole rollout is ONE
 * persistent kernel (state resident on-chip across steps); so is the classical
 * rollout (model == NULL) at nx <= 64 and nx in {256, 512, 1024}, bit-identical to T
 * hf_step calls (HF_FV_PERSIST=0 in the environment selects the per-step
 * launches, for A/B timing).  Otherwise, with
 * model != NULL and B*nx >= 2^21 cells, slices of the batch step on up to 3
 * library-owned lane streams forked from and joined back into `stream` with
 * events (HF_RUN_LANES=1..4 in the environment overrides the count): the call
 * stays ordered on `stream` (and capturable), and every IC's result is
 * bit-identical to the one-stream sequencing.  The lane streams belong to
 * (device, `stream`): calls on different streams or threads never share a
 * lane, and capturing `stream` draws in only its own lanes.
 */
int hf_run(hf_model_t model, const float *dev_state0, float *dev_state_final,
           const float *dev_x, const double *dev_c, int B, int nx, int T,
           float c, float dt, float nu, float dx2,
           float *dev_traj, float *dev_flux_traj, float *dev_metrics,
           void *dev_workspace, int64_t workspace_bytes, void *stream);
/* hf_run with a Poisson mode; same paths, workspace and aliasing rules. */
int hf_run_ex(hf_model_t model, const float *dev_state0, float *dev_state_final,
              const float *dev_x, const double *dev_plan, int poisson_mode, int B, int nx, int T,
              float c, float dt, float nu, float dx2,
              float *dev_traj, float *dev_flux_traj, float *dev_metrics,
              void *dev_workspace, int64_t workspace_bytes, void *stream);

/*
 * Coarse-grained fine classical rollouts: the "fine reference" of the
 * reference README's claims ("matches fine-step baseline on coarse grid",
 * "larger time steps (2-5x)"), which neither scripts/training/generate_data.py
 * nor the evaluation scripts can produce: they run the classical solver on the
 * training grid at the training step.  Here the classical solver runs on
 * refine (r) x the cells with substeps (S) x smaller steps, and its states and
 * face fluxes are reduced to the coarse grid (nx = nx_f / r, dt = S dt_f).
 *
 * hf_coarsen_traj is the definition.  From a recorded fine trajectory
 * dev_traj_f [B][T_f+1][3][nx_f] and (optionally, both or neither) the fine
 * flux dev_flux_f [B][T_f][nx_f], with T_c = T_f / S (T_f % S == 0):
 *   dev_traj_c [B][T_c+1][3][nx_f/r]: for each of n, u, E the value
 *     (float)(tree / r), tree the ADJACENT PAIRWISE float64 sum of the r
 *     float32 cells r j .. r j + r - 1 of fine row S t_c (level 1 adds cells
 *     (2m, 2m+1), level 2 adds those sums pairwise, ...);
 *   dev_flux_c [B][T_c][nx_f/r]: (float)(acc / S), acc the float64 sum, in
 *     ascending substep order from 0.0, of the fine F at cell r j + r - 1 (the
 *     right face of coarse cell j; F_i = n_i u_i is the flux through face
 *     i + 1/2) over fine steps S t_c .. S t_c + S - 1; a float64 division.
 * r = 1 copies the states bit for bit.  The time-averaged flux is the flux a
 * coarse finite-volume step needs to be exact:
 *   nbar_j' = nbar_j - (dt/dx) (Fbar_j - Fbar_{j-1}),  dt = S dt_f, dx = r dx_f,
 * holds to rounding ((3 S + 4) float32 ulps of max|n| + 2 c_f max|F|).
 * refine: a power of two in 1..64 that divides nx_f; substeps >= 1.
 *
 * hf_run_coarse is hf_coarsen_traj(hf_run_ex(model = NULL, traj, flux)) bit
 * for bit, without the fine trajectory in HBM.  c, dt, nu, dx2, dev_plan and
 * poisson_mode are the FINE grid's (c = f32(dt_f/dx_f), ...); dev_state0 is
 * fine [B][3][nx_f].  Outputs, each may be NULL but not all three:
 *   dev_traj  [B][T_c+1][3][nx_f/r]  coarse, row 0 = the coarsened IC;
 *   dev_flux  [B][T_c][nx_f/r]       coarse;
 *   dev_state_final [B][3][nx_f]     FINE, so a rollout can be continued (may
 *                                    alias dev_state0).
 * Where hf_run is one launch (nx_f <= 64 and nx_f in {256, 512, 1024}) so is
 * this: the fine states stay in registers, a coarse cell's r fine cells sit
 * in r adjacent lanes, the box sum is an xor butterfly over lane distances
 * 1 .. r/2 in float64 (exactly the pairwise tree), and only coarse rows and
 * fluxes are stored, every S steps; no workspace.  Any other nx_f sequences
 * hf_run_ex over chunks of coarse steps into the workspace and coarsens each
 * chunk; the result does not depend on the chunking.
 * hf_run_coarse_workspace_bytes(B, nx_f, T_c, r, S): the bytes with which T_c
 * coarse steps run as ONE chunk (0 on the one-launch paths, for B = 0 and for
 * T_c = 0; -1 on bad arguments).  A call given fewer bytes runs chunks of the
 * most coarse steps whose query fits; fewer than the query at T_c = 1 is
 * HF_EINVAL.  dev_workspace == NULL: the call allocates stream-ordered, at
 * most 256 MiB (but always one coarse step's worth).
 * HF_EINVAL, before any device call: refine not a power of two in 1..64 or
 * not dividing nx_f, substeps < 1, T_c < 0 (T_f % substeps != 0), no output
 * requested, a workspace too small.  B = 0 and T_c = 0 are HF_OK (row 0 is
 * written).  Both Poisson modes, as hf_run_ex.
 */
int hf_coarsen_traj(const float *dev_traj_f, const float *dev_flux_f /* or NULL */, int B, int nx_f, int T_f,
                    int refine, int substeps, float *dev_traj_c, float *dev_flux_c /* or NULL */, void *stream);
int64_t hf_run_coarse_workspace_bytes(int B, int nx_f, int T_c, int refine, int substeps);
int hf_run_coarse(const float *dev_state0, float *dev_state_final /* or NULL */, const double *dev_plan,
                  int poisson_mode, int B, int nx_f, int T_c, int refine, int substeps,
                  float c, float dt, float nu, float dx2,
                  float *dev_traj /* or NULL */, float *dev_flux /* or NULL */,
                  void *dev_workspace, int64_t workspace_bytes, void *stream);

/*
 * Hybrid rollout scored against the classical solver from the same ICs, in
 * one pass (replaces the serial per-IC loop of
 * scripts/evaluation/evaluate_multi_ic.py:21-94: BaselineSolver.step from
 * state0, HybridSolver.run from state0, per-step channel MSE; and the
 * energy/charge series of scripts/evaluation/evaluate_all.py:118-159).
 * The classical twin uses the same dt/dx and viscosity `nu`.
 * dev_mse [B][T+1][3] float32 (required): mean over cells of
 *   (hybrid - classical)^2 for n, u, E at every step (step 0 is 0), summed in
 *   float64 and rounded once.
 * dev_metrics / dev_metrics_classical [B][T+1][HF_NUM_METRICS] (may be NULL).
 * dev_state_final receives the hybrid final state; it may alias dev_state0.
 * For nx in {16,32,48,64} both solvers advance inside the one persistent kernel.
 * For nx in {256, 512, 1024} (model not fused) the hybrid rollout runs first and
 * the classical twin is one launch that scores each step against the hybrid
 * trajectory as it goes; the results equal the recorded-trajectory path bit
 * for bit.  dev_workspace, if given, is sized by hf_workspace_need(model,
 * HF_OP_COMPARE, ...): 0 at the fused nx, one hybrid trajectory plus the face
 * flux at nx in {256, 512, 1024}, two trajectories, a state and the flux
 * otherwise.
 */
int hf_run_compare(hf_model_t model, const float *dev_state0, float *dev_state_final,
                   const float *dev_x, const double *dev_c, int B, int nx, int T,
                   float c, float dt, float nu, float dx2, float *dev_mse,
                   float *dev_metrics, float *dev_metrics_classical,
                   void *dev_workspace, int64_t workspace_bytes, void *stream);
/* hf_run_compare with a Poisson mode: the hybrid rollout AND its classical
 * twin both use it. */
int hf_run_compare_ex(hf_model_t model, const float *dev_state0, float *dev_state_final,
                      const float *dev_x, const double *dev_plan, int poisson_mode, int B, int nx, int T,
                      float c, float dt, float nu, float dx2, float *dev_mse,
                      float *dev_metrics, float *dev_metrics_classical,
                      void *dev_workspace, int64_t workspace_bytes, void *stream);

/*
 * Model sets: M FluxGNN checkpoints rolled out in one launch (an ablation
 * sweep's models, or an ensemble's members, from the same or their own ICs).
 * hf_model_set_create: M >= 1 models of one wdtype, on the current device; all
 * chain-capable (in_dim 4, hidden 128) or the call is HF_EUNSUPPORTED.  Uploads
 * the table of their weights' addresses once; the models must outlive the set.
 * Their `layers` may differ.
 */
typedef struct hf_model_set *hf_model_set_t;
int hf_model_set_create(const hf_model_t *models, int M, hf_model_set_t *out);
void hf_model_set_destroy(hf_model_set_t set);
int hf_model_set_size(hf_model_set_t set); /* M; 0 for NULL */
/*
 * hf_run_ex / hf_run_compare_ex for every model of the set.  model_stride, in
 * floats, says where model m's ICs start (dev_state0 + m*model_stride): 0 =
 * all M models start from the same [B][3][nx] states, B*3*nx = dev_state0 is
 * [M][B][3][nx]; any other value is HF_EINVAL.  Every output is model-major:
 * dev_state_final [M][B][3][nx], dev_traj [M][B][T+1][3][nx], dev_flux_traj
 * [M][B][T][nx], dev_metrics / dev_metrics_classical [M][B][T+1][HF_NUM_METRICS],
 * dev_mse [M][B][T+1][3]; each model's block holds exactly what the
 * single-model call writes for it, bit for bit.  dev_state_final may alias
 * dev_state0 only when model_stride != 0 (with shared ICs: HF_EINVAL).
 * For nx in {16,32,48,64} the call is ONE persistent launch of M x G
 * workgroups (G = one model's workgroup count), each workgroup serving the
 * model blockIdx.x / G: no allocation, no host synchronisation, capturable.
 * For any other nx the M models run one after another on `stream` through the
 * single-model sequencing; dev_workspace is then sized by
 * hf_set_workspace_need (the largest single-model need; op HF_OP_RUN or
 * HF_OP_COMPARE, flags as hf_workspace_need; -1 on bad arguments), and M*B
 * must fit an int.
 */
int hf_run_set(hf_model_set_t set, const float *dev_state0, int64_t model_stride,
               float *dev_state_final, const float *dev_x, const double *dev_plan,
               int poisson_mode, int B, int nx, int T, float c, float dt, float nu, float dx2,
               float *dev_traj, float *dev_flux_traj, float *dev_metrics,
               void *dev_workspace, int64_t workspace_bytes, void *stream);
int hf_run_compare_set(hf_model_set_t set, const float *dev_state0, int64_t model_stride,
                       float *dev_state_final, const float *dev_x, const double *dev_plan,
                       int poisson_mode, int B, int nx, int T, float c, float dt, float nu, float dx2,
                       float *dev_mse, float *dev_metrics, float *dev_metrics_classical,
                       void *dev_workspace, int64_t workspace_bytes, void *stream);
int64_t hf_set_workspace_need(hf_model_set_t set, int op, int B, int nx, int T, int flags);

/*
 * Metric series of recorded trajectories (the host-side scoring of
 * scripts/evaluation/evaluate_all.py:118-159 and evaluate_multi_ic.py:88-94,
 * on the device):
 * hf_traj_metrics: dev_traj [B][T1][3][nx] -> dev_metrics [B][T1][HF_NUM_METRICS].
 * hf_traj_mse: per-step channel MSE of two trajectories [B][T1][3][nx] ->
 *   dev_mse [B][T1][3] (n, u, E), float64 sums rounded once.
 */
int hf_traj_metrics(const float *dev_traj, int B, int T1, int nx, float *dev_metrics, void *stream);
int hf_traj_mse(const float *dev_traj_a, const float *dev_traj_b, int B, int T1, int nx, float *dev_mse,
                void *stream);

/*
 * Scored rollouts of the comparison models.  Replace
 * scripts/evaluation/evaluate_multi_ic.py:21-94 for model types 'pure_gnn'
 * (:45-66) and 'pinn' (:70-83) — the model's rollout, BaselineSolver.run from
 * the same IC (:28-33) and the per-step channel MSE (:88-94) — and the
 * explosion / energy-drift series of evaluate_long_rollout.py:18-81, for B ICs
 * in one call: hf_pure_gnn_run / hf_pinn_run (same dev_final and dev_traj, bit
 * for bit) that also write
 *   dev_metrics           [B][T+1][HF_NUM_METRICS]  = hf_traj_metrics(model trajectory),
 *   dev_mse               [B][T+1][3]               = hf_traj_mse(model, classical trajectory),
 *   dev_metrics_classical [B][T+1][HF_NUM_METRICS]  = hf_run(model = NULL)'s metrics,
 * each bit for bit, without either trajectory going through memory.  dev_traj,
 * dev_metrics, dev_mse and dev_metrics_classical may each be NULL; the
 * classical twin (dt, nu, c = dt/dx, dx2 = dx^2, dev_plan of poisson_mode: the
 * arguments of hf_run_ex) runs exactly when dev_mse is given.
 * dev_metrics_classical without dev_mse, and dev_metrics and dev_mse both NULL
 * (nothing to score), are HF_EINVAL; so are NULL required pointers (dev_plan
 * is required with dev_mse), negative sizes, an unknown Poisson mode, for PINN
 * dim % 3 != 0 (nx = dim / 3) or layers outside 2..8, and a workspace_bytes
 * below hf_*_score_workspace_bytes (-1 on bad arguments) or a NULL workspace
 * where that is > 0 — all before any device call.  dev_final may alias
 * dev_state0.
 *
 * One launch on PureGNN hidden in {64, 128} with nx in {16, 32, 48, 64} and on
 * PINN(192, 256, 2..8), any T >= 0: one wave per IC scores the state held in
 * LDS and keeps the twin in registers; the workspace is what the unscored
 * rollout needs.  Every other shape sequences the existing kernels (the
 * model's rollout into a trajectory in the workspace, the classical hf_run
 * into a second, hf_traj_metrics, hf_traj_mse), as hf_run_compare does for its
 * generic nx; the workspace holds both trajectories.
 */
int64_t hf_pure_gnn_score_workspace_bytes(int hidden, int B, int nx, int T);
int hf_pure_gnn_run_scored(const float *dev_params, int hidden, int layers, const float *dev_state0,
                           float *dev_state_final, const float *dev_x, const double *dev_plan, int poisson_mode,
                           int B, int nx, int T, float c, float dt, float nu, float dx2, float *dev_traj,
                           float *dev_metrics, float *dev_mse, float *dev_metrics_classical, void *dev_workspace,
                           int64_t workspace_bytes, void *stream);
int64_t hf_pinn_score_workspace_bytes(int dim, int hidden, int64_t B, int T);
int hf_pinn_run_scored(const float *dev_params, int dim, int hidden, int layers, const float *dev_state0,
                       float *dev_state_final, const double *dev_plan, int poisson_mode, int64_t B, int T, float c,
                       float dt, float nu, float dx2, float *dev_traj, float *dev_metrics, float *dev_mse,
                       float *dev_metrics_classical, void *dev_workspace, int64_t workspace_bytes, void *stream);

/*
 * Per-IC summary of a T-step rollout from its metric series (SURVEY.md 8f
 * rank 1; fields at HF_NUM_SUMMARY).  dev_metrics [B][T+1][HF_NUM_METRICS]
 * (required), dev_mse [B][T+1][3] (may be NULL), dev_metrics_ref
 * [B][T+1][HF_NUM_METRICS] (may be NULL: the classical twin's series).
 * dev_summary [B][HF_NUM_SUMMARY] (required); dev_drift [B][T+1][4] (may be
 * NULL): |energy_t - energy_0|, |charge_t - charge_0| of the rollout, then
 * of the reference series (NaN without one).
 */
int hf_rollout_summary(const float *dev_metrics, const float *dev_mse, const float *dev_metrics_ref, int B,
                       int T, float *dev_summary, float *dev_drift, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* HYBRIDFLUX_H */
