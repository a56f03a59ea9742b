// Host-sanitized drive of every size query of the C ABI that takes no handle.
//
// Built by `make -C gnn-plasma-flux_amd/csrc asan-workspace` with
// AddressSanitizer and UBSan on the HOST code only.  A size query runs the code
// that carves the buffer on a NULL base (hf_internal.h Carve), so this is the
// NULL-base check: UBSan reports any arithmetic a layout does on a NULL
// pointer.  Every query is called over the shapes of tests/workspace_sizes.json
// (tools/dump_workspace_sizes.py) and over huge ones; a result is a size or -1,
// and a size does not shrink as the batch grows.  Needs no device.  Exit 0 = clean.
#include <cstdint>

#include "expect.h"

static const int kB[] = {0, 1, 3, 64, 1029, 4096};
static const int kNx[] = {1, 16, 48, 63, 64, 100, 256, 1024, 2048, 6145};
static const int kT[] = {0, 1, 30};
static const int kHidden[] = {32, 64, 128, 256};
static const int kLayers[] = {0, 1, 4, 8};
static const int kInDim[] = {1, 4, 8};
static const int kPinn[][2] = {{192, 256}, {48, 64}, {3, 32}, {300, 32}, {300, 128}, {3 * 6145, 256}};
static const int kCoarse[][2] = {{1, 1}, {4, 2}, {64, 3}};
static const int kI31 = INT32_MAX;

static void valid(const char *name, int64_t v) {
  if (v < -1) std::fprintf(stderr, "%s returned %lld\n", name, (long long)v);
  EXPECT(v >= -1);
}

// One query with its other arguments fixed, as a function of the batch.
template <class F>
static void sweep(const char *name, F f) {
  int64_t last = -1;
  for (int B : kB) {
    const int64_t v = f(B);
    valid(name, v);
    if (v < 0) continue;
    if (v < last) std::fprintf(stderr, "%s shrinks at B = %d: %lld < %lld\n", name, B, (long long)v, (long long)last);
    EXPECT(v >= last);
    last = v;
  }
  valid(name, f(-1));
}

typedef int64_t (*BNx)(int, int);
typedef int64_t (*Gnn)(int, int, int, int64_t, int64_t);

int main() {
  const struct {
    const char *name;
    BNx q;
  } bnx[] = {{"hf_ablation_loss_workspace_bytes", hf_ablation_loss_workspace_bytes},
             {"hf_unroll_workspace_bytes", hf_unroll_workspace_bytes},
             {"hf_unroll_workspace_bytes_ex", hf_unroll_workspace_bytes_ex},
             {"hf_pure_unroll_workspace_bytes", hf_pure_unroll_workspace_bytes},
             {"hf_pure_unroll_workspace_bytes_ex", hf_pure_unroll_workspace_bytes_ex},
             {"hf_pinn_unroll_workspace_bytes", hf_pinn_unroll_workspace_bytes},
             {"hf_pinn_unroll_workspace_bytes_ex", hf_pinn_unroll_workspace_bytes_ex},
             {"hf_pinn_loss_workspace_bytes", hf_pinn_loss_workspace_bytes},
             {"hf_state_mse_workspace_bytes", hf_state_mse_workspace_bytes}};
  for (const auto &q : bnx) {
    for (int nx : kNx) sweep(q.name, [&](int B) { return q.q(B, nx); });
    EXPECT(q.q(1, 0) == -1 && q.q(kI31, -1) == -1);
    valid(q.name, q.q(kI31, 1 << 20));
  }
  EXPECT(hf_state_mse_workspace_bytes(65536, 65536) == -1);  // 3 B nx past int
  EXPECT(hf_pure_unroll_workspace_bytes(kI31, kI31) == -1 && hf_pure_unroll_workspace_bytes_ex(kI31, kI31) == -1);
  for (BNx q : {hf_unroll_workspace_bytes_ex, hf_pinn_unroll_workspace_bytes_ex, hf_pinn_loss_workspace_bytes})
    EXPECT(q(kI31, kI31) > 8LL * kI31);

  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)66049, (int64_t)1 << 40})
    valid("hf_adam_flat_workspace_bytes", hf_adam_flat_workspace_bytes(n));
  EXPECT(hf_adam_flat_workspace_bytes(-1) == -1);

  const struct {
    const char *name;
    Gnn q;
    int min_n;  // hf_graph_backward_workspace_bytes: N = 0 is not asked (tools/dump_workspace_sizes.py)
  } gnn[] = {{"hf_graph_tape_bytes", hf_graph_tape_bytes, 0},
             {"hf_graph_backward_workspace_bytes", hf_graph_backward_workspace_bytes, 1},
             {"hf_pure_gnn_tape_bytes", hf_pure_gnn_tape_bytes, 0},
             {"hf_pure_gnn_backward_workspace_bytes", hf_pure_gnn_backward_workspace_bytes, 0}};
  for (const auto &q : gnn) {
    for (int in : kInDim)
      for (int h : kHidden)
        for (int l : kLayers)
          for (int nx : {16, 63, 100, 6145})
            for (int e = 0; e < 2; ++e)
              sweep(q.name, [&](int B) {
                const int64_t N = (int64_t)B * nx;
                return N < q.min_n ? (int64_t)-1 : q.q(in, h, l, N, e ? 3 * N + 1 : 2 * N);
              });
    EXPECT(q.q(4, 128, 9, 64, 128) == -1 && q.q(0, 128, 4, 64, 128) == -1 && q.q(4, 128, 4, 64, -1) == -1);
    valid(q.name, q.q(8, 256, 8, (int64_t)1 << 36, (int64_t)1 << 37));
    valid(q.name, q.q(4, 128, 8, (int64_t)1 << 36, (int64_t)1 << 37));
  }
  for (int h : kHidden)
    for (int nx : kNx) {
      for (int e = 0; e < 2; ++e)
        sweep("hf_pure_gnn_workspace_bytes", [&](int B) {
          const int64_t N = (int64_t)B * nx;
          return hf_pure_gnn_workspace_bytes(h, N, e ? 3 * N + 1 : 2 * N);
        });
      for (int T : kT) {
        sweep("hf_pure_gnn_run_workspace_bytes", [&](int B) { return hf_pure_gnn_run_workspace_bytes(h, B, nx, T); });
        sweep("hf_pure_gnn_score_workspace_bytes", [&](int B) { return hf_pure_gnn_score_workspace_bytes(h, B, nx, T); });
      }
    }
  valid("hf_pure_gnn_workspace_bytes", hf_pure_gnn_workspace_bytes(256, (int64_t)1 << 40, (int64_t)1 << 41));
  EXPECT(hf_pure_gnn_workspace_bytes(0, 64, 128) == -1 && hf_pure_gnn_run_workspace_bytes(128, 1, 0, 1) == -1);
  valid("hf_pure_gnn_run_workspace_bytes", hf_pure_gnn_run_workspace_bytes(32, 1 << 20, 1 << 20, 1 << 20));
  EXPECT(hf_pure_gnn_score_workspace_bytes(32, 1 << 20, 1 << 20, 1 << 20) == -1);  // a trajectory past 2^60 bytes

  for (const auto &p : kPinn) {
    sweep("hf_pinn_workspace_bytes", [&](int B) { return hf_pinn_workspace_bytes(p[0], p[1], B); });
    for (int l : {1, 2, 4, 8, 9}) {
      sweep("hf_pinn_tape_bytes", [&](int B) { return hf_pinn_tape_bytes(p[0], p[1], l, B); });
      sweep("hf_pinn_backward_workspace_bytes", [&](int B) { return hf_pinn_backward_workspace_bytes(p[0], p[1], l, B); });
    }
    for (int T : kT) sweep("hf_pinn_score_workspace_bytes", [&](int B) { return hf_pinn_score_workspace_bytes(p[0], p[1], B, T); });
    valid("hf_pinn_workspace_bytes", hf_pinn_workspace_bytes(p[0], p[1], (int64_t)1 << 40));
    valid("hf_pinn_tape_bytes", hf_pinn_tape_bytes(p[0], p[1], 8, kI31));
    valid("hf_pinn_backward_workspace_bytes", hf_pinn_backward_workspace_bytes(p[0], p[1], 8, kI31));
  }
  EXPECT(hf_pinn_tape_bytes(192, 256, 4, (int64_t)kI31 + 1) == -1 && hf_pinn_tape_bytes(65537, 256, 4, 1) == -1);
  EXPECT(hf_pinn_backward_workspace_bytes(192, 256, 4, (int64_t)kI31 + 1) == -1);
  EXPECT(hf_pinn_score_workspace_bytes(300, 32, (int64_t)1 << 40, 1 << 30) == -1);  // a trajectory past 2^60 bytes
  EXPECT(hf_pinn_score_workspace_bytes(191, 256, 1, 1) == -1);

  for (int nx : kNx)
    for (int T : kT) {
      for (int op : {HF_OP_STEP, HF_OP_RUN, HF_OP_COMPARE}) {
        sweep("hf_run_workspace_bytes", [&](int B) { return hf_run_workspace_bytes(op, B, nx, T); });
        for (int flags = 0; flags < 4; ++flags)
          sweep("hf_workspace_need", [&](int B) { return hf_workspace_need(nullptr, op, B, nx, T, flags); });
      }
      for (const auto &c : kCoarse)
        sweep("hf_run_coarse_workspace_bytes", [&](int B) { return hf_run_coarse_workspace_bytes(B, nx, T, c[0], c[1]); });
    }
  EXPECT(hf_run_workspace_bytes(3, 1, 16, 1) == -1 && hf_workspace_need(nullptr, HF_OP_RUN, 1, 16, 1, 4) == -1);
  valid("hf_run_workspace_bytes", hf_run_workspace_bytes(HF_OP_COMPARE, 1 << 20, 1 << 20, 1 << 10));
  valid("hf_workspace_need", hf_workspace_need(nullptr, HF_OP_RUN, 1 << 20, 6145, 1 << 10, 0));
  EXPECT(hf_run_coarse_workspace_bytes(1, 6145, kI31, 1, 2) == -1);       // T_c * substeps past int
  EXPECT(hf_run_coarse_workspace_bytes(kI31, kI31, kI31, 1, 1) == -1);    // more bytes than int64 holds
  EXPECT(hf_run_coarse_workspace_bytes(1, 64, 1, 3, 1) == -1 && hf_run_coarse_workspace_bytes(1, 64, 1, 1, 0) == -1);
  return finish("workspace_sanitize");
}
