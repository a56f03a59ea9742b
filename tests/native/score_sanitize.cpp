// Host-sanitized drive of the scored-rollout entry points of the C ABI
// (hf_pure_gnn_score_workspace_bytes, hf_pure_gnn_run_scored,
// hf_pinn_score_workspace_bytes, hf_pinn_run_scored).
//
// Built by `make -C gnn-plasma-flux_amd/csrc asan-score` with AddressSanitizer
// and UBSan on the HOST code only, like unroll_sanitize.cpp.  It walks the
// validation paths: every call must be refused (HF_EINVAL, or HF_EUNSUPPORTED
// for a Poisson mode the shape does not support) before any device call, so
// they need no device and launch nothing; the dummy device pointers are never
// dereferenced.  Exit 0 = clean.
#include <cstdint>

#include "expect.h"

struct Args {
  float *params = reinterpret_cast<float *>(16), *s0 = reinterpret_cast<float *>(32);
  float *fin = reinterpret_cast<float *>(48), *x = reinterpret_cast<float *>(64);
  double *plan = reinterpret_cast<double *>(80);
  float *traj = reinterpret_cast<float *>(96), *met = reinterpret_cast<float *>(112);
  float *mse = reinterpret_cast<float *>(128), *mcl = reinterpret_cast<float *>(144);
  void *ws = reinterpret_cast<void *>(256);
  int pm = HF_POISSON_SPECTRAL;
  int hidden = 128, layers = 4, B = 3, nx = 64, T = 5;  // PureGNN: a one-launch shape
  int dim = 192, phidden = 256, players = 4;             // PINN: the one-launch shape
  int64_t ws_short = 0;
};

static int pure(const Args &a) {
  int64_t nb = hf_pure_gnn_score_workspace_bytes(a.hidden, a.B, a.nx, a.T);
  if (nb < 0) nb = 1 << 20;
  return hf_pure_gnn_run_scored(a.params, a.hidden, a.layers, a.s0, a.fin, a.x, a.plan, a.pm, a.B, a.nx, a.T, 0.05f,
                                5e-3f, 1e-3f, 0.01f, a.traj, a.met, a.mse, a.mcl, a.ws, nb - a.ws_short, nullptr);
}
static int pinn(const Args &a) {
  int64_t nb = hf_pinn_score_workspace_bytes(a.dim, a.phidden, a.B, a.T);
  if (nb < 0) nb = 1 << 20;
  return hf_pinn_run_scored(a.params, a.dim, a.phidden, a.players, a.s0, a.fin, a.plan, a.pm, a.B, a.T, 0.05f, 5e-3f,
                            1e-3f, 0.01f, a.traj, a.met, a.mse, a.mcl, a.ws, nb - a.ws_short, nullptr);
}

int main() {
  // size queries: the unscored need on the one-launch shapes, two trajectories more elsewhere, -1 on bad arguments
  EXPECT(hf_pure_gnn_score_workspace_bytes(128, 3, 64, 5) == hf_pure_gnn_run_workspace_bytes(128, 3, 64, 5));
  EXPECT(hf_pure_gnn_score_workspace_bytes(64, 3, 16, 0) == 0);
  EXPECT(hf_pure_gnn_score_workspace_bytes(64, 2, 20, 5) >=
         hf_pure_gnn_run_workspace_bytes(64, 2, 20, 5) + 2LL * 4 * 2 * 6 * 3 * 20);
  EXPECT(hf_pure_gnn_score_workspace_bytes(64, 1 << 20, 20, 1 << 20) > (1LL << 40));
  EXPECT(hf_pure_gnn_score_workspace_bytes(64, INT32_MAX, 20, INT32_MAX) == -1);  // > 2^60 bytes; no int overflow (UBSan)
  EXPECT(hf_pure_gnn_score_workspace_bytes(0, 3, 64, 5) == -1);
  EXPECT(hf_pure_gnn_score_workspace_bytes(64, -1, 64, 5) == -1);
  EXPECT(hf_pure_gnn_score_workspace_bytes(64, 3, 0, 5) == -1);
  EXPECT(hf_pure_gnn_score_workspace_bytes(64, 3, 64, -1) == -1);
  EXPECT(hf_pure_gnn_score_workspace_bytes(INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN) == -1);
  EXPECT(hf_pinn_score_workspace_bytes(192, 256, 17, 5) == hf_pinn_workspace_bytes(192, 256, 17));
  EXPECT(hf_pinn_score_workspace_bytes(48, 32, 3, 5) >= hf_pinn_workspace_bytes(48, 32, 3) + 2LL * 4 * 3 * 6 * 48);
  EXPECT(hf_pinn_score_workspace_bytes(48, 32, 1LL << 40, INT32_MAX) == -1);  // > 2^60 bytes
  EXPECT(hf_pinn_score_workspace_bytes(50, 32, 3, 5) == -1);  // dim % 3
  EXPECT(hf_pinn_score_workspace_bytes(0, 32, 3, 5) == -1);
  EXPECT(hf_pinn_score_workspace_bytes(48, 0, 3, 5) == -1);
  EXPECT(hf_pinn_score_workspace_bytes(48, 32, -1, 5) == -1);
  EXPECT(hf_pinn_score_workspace_bytes(48, 32, 3, -1) == -1);

  const char *pg = "hf_pure_gnn_run_scored", *pn = "hf_pinn_run_scored";
  for (int which = 0; which < 2; ++which) {
    auto call = which ? pinn : pure;
    const char *fn = which ? pn : pg;
    {  // required pointers (the plan with dev_mse only)
      float *Args::*req[] = {&Args::params, &Args::s0, &Args::fin};
      for (auto m : req) {
        Args a;
        a.*m = nullptr;
        EXPECT(call(a) == HF_EINVAL && named(fn));
      }
      Args a;
      a.plan = nullptr;
      EXPECT(call(a) == HF_EINVAL && named(fn));
      a = Args();
      a.ws = nullptr;
      EXPECT(call(a) == HF_EINVAL && named(fn));
      a = Args();
      a.ws_short = 1;  // one byte short
      EXPECT(call(a) == HF_EINVAL && named(fn));
    }
    {  // what to score
      Args a;
      a.met = a.mse = a.mcl = nullptr;  // nothing
      EXPECT(call(a) == HF_EINVAL && named(fn));
      a = Args();
      a.mse = nullptr;  // the twin's metrics without the twin
      EXPECT(call(a) == HF_EINVAL && named(fn));
      a = Args();
      a.B = 0, a.met = a.mse = nullptr;  // refused before the empty batch returns
      EXPECT(call(a) == HF_EINVAL && named(fn));
    }
    {  // sizes and the Poisson mode
      Args a;
      a.B = -1;
      EXPECT(call(a) == HF_EINVAL && named(fn));
      for (int T : {-1, INT32_MIN}) {
        a = Args();
        a.T = T;
        EXPECT(call(a) == HF_EINVAL && named(fn));
      }
      for (int pm : {-1, 2, INT32_MAX}) {
        a = Args();
        a.pm = pm;
        EXPECT(call(a) == HF_EINVAL && named(fn));
      }
    }
  }
  {  // PureGNN only: x, the model and chain sizes; a shape without a one-launch kernel
    Args a;
    a.x = nullptr;
    EXPECT(pure(a) == HF_EINVAL && named(pg));
    for (int v : {0, -1, INT32_MIN}) {
      a = Args();
      a.hidden = v;
      EXPECT(pure(a) == HF_EINVAL && named(pg));
      a = Args();
      a.nx = v;
      EXPECT(pure(a) == HF_EINVAL && named(pg));
    }
    a = Args();
    a.layers = -1;
    EXPECT(pure(a) == HF_EINVAL && named(pg));
    a = Args();
    a.nx = 20, a.ws_short = 1;
    EXPECT(pure(a) == HF_EINVAL && named(pg));
    a = Args();
    a.nx = 20, a.mse = nullptr;
    EXPECT(pure(a) == HF_EINVAL && named(pg));
    a = Args();
    a.nx = 20000, a.pm = HF_POISSON_TRIDIAG;  // the tridiagonal twin's nx limit
    EXPECT(pure(a) == HF_EUNSUPPORTED && named(pg));
  }
  {  // PINN only: dim = 3 nx, layers 2..8
    Args a;
    for (int d : {50, 191, 0, -3}) {
      a = Args();
      a.dim = d;
      EXPECT(pinn(a) == HF_EINVAL && named(pn));
    }
    for (int l : {1, 9, -1}) {
      a = Args();
      a.players = l;
      EXPECT(pinn(a) == HF_EINVAL && named(pn));
    }
    a = Args();
    a.phidden = 0;
    EXPECT(pinn(a) == HF_EINVAL && named(pn));
    a = Args();
    a.dim = 48, a.phidden = 32, a.ws_short = 1;  // no one-launch kernel: the workspace holds two trajectories
    EXPECT(pinn(a) == HF_EINVAL && named(pn));
  }
  return finish("score_sanitize");
}
