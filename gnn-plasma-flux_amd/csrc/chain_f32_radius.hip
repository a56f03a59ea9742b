// The f32 chain core at stencil radius 2 and 3: FluxGNN on the radius-R chain
// graph (for r = 1..R the edges i -> i+r and i+r -> i, mean over the 2R
// neighbours), whose first 2 nx edges per IC, the reference's, feed the solver.
//
// Replaces: nothing the reference runs: its radius names a checkpoint
// (src/hybrid_solver.py:32) and its graph is always the ±1 chain
// (src/graph_constructor.py:34-38).
//
// The core is chain_f32.hip's CoreF32T with RAD = 2, 3 (included here alone):
// the B operand's second half is the 2R-term neighbour sum in edge-list order
// (chain_common.h nb_sum_radius), W_b arrives packed as w / (2R), and the
// windowed flux kernel's halo is L*R cells.  A translation unit of its own: the
// radius-1 object is what it was and the two build side by side.  The
// cell-split kernels stay radius 1, so small batches run IC-per-wave here.
#define HF_CHAIN_F32_CORE_ONLY
#include "chain_f32.hip"

namespace hf {
namespace {
using CoreF32R2 = CoreF32T<2, kRingSlots, false, true, 2>;
using CoreF32R3 = CoreF32T<2, kRingSlots, false, true, 3>;
}  // namespace

hipError_t launch_chain_flux_f32_radius(const ChainW &w, const float *nf, const float *state, int64_t ld_state,
                                        const float *x, int B, int nx, float *fe, float *ff, hipStream_t s) {
  if (nx < 2 * w.radius + 1) return hipErrorInvalidValue;  // an edge would repeat
  switch (w.radius) {
    case 2: return chain::launch_flux_core<CoreF32R2>(w, nf, state, ld_state, x, B, nx, fe, ff, s);
    case 3: return chain::launch_flux_core<CoreF32R3>(w, nf, state, ld_state, x, B, nx, fe, ff, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_chain_rollout_f32_radius(const ChainW &w, const float *state0, float *state_final, const float *x,
                                           const double *pc, int B, int nx, int T, float c, float dt, float *traj,
                                           float *flux_traj, float *metrics, const RolloutExtras &ex, hipStream_t s) {
  switch (w.radius) {
    case 2:
      return chain::launch_rollout_core<CoreF32R2>(w, state0, state_final, x, pc, B, nx, T, c, dt, traj, flux_traj,
                                                   metrics, ex, s);
    case 3:
      return chain::launch_rollout_core<CoreF32R3>(w, state0, state_final, x, pc, B, nx, T, c, dt, traj, flux_traj,
                                                   metrics, ex, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_chain_rollout_set_f32_radius(const ChainSet &set, const float *state0, float *state_final,
                                               const float *x, const double *pc, int B, int nx, int T, float c,
                                               float dt, float *traj, float *flux_traj, float *metrics,
                                               const RolloutExtras &ex, hipStream_t s) {
  switch (set.radius) {
    case 2:
      return chain::launch_rollout_core_set<CoreF32R2>(set, state0, state_final, x, pc, B, nx, T, c, dt, traj,
                                                       flux_traj, metrics, ex, s);
    case 3:
      return chain::launch_rollout_core_set<CoreF32R3>(set, state0, state_final, x, pc, B, nx, T, c, dt, traj,
                                                       flux_traj, metrics, ex, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace hf
