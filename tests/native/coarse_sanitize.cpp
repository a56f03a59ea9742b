// Host-sanitized drive of the coarse-grained rollout entry points of the C ABI
// (hf_coarsen_traj, hf_run_coarse, hf_run_coarse_workspace_bytes).
//
// Built by `make -C gnn-plasma-flux_amd/csrc asan-coarse` with AddressSanitizer
// and UBSan on the HOST code only, like cons_sanitize.cpp.  It walks the
// validation paths: every call in the first part must be refused with HF_EINVAL
// before any device call, so those need no device and launch nothing; the dummy
// device pointers are never dereferenced.  The last part hands valid arguments:
// on a machine without a device the launch itself fails and the call returns
// HF_EHIP (on one with a device the dummy pointers would be dereferenced, so
// that part is skipped there).  Exit 0 = clean.
#include <cstdint>

#include "expect.h"

static float *fp(uintptr_t v) { return reinterpret_cast<float *>(v); }

struct Args {
  float *st = fp(16), *fin = fp(32), *traj = fp(48), *flux = fp(64);
  double *plan = reinterpret_cast<double *>(96);
  void *ws = reinterpret_cast<void *>(256);
  int64_t ws_bytes = -1;  // -1: the one-chunk size
  int pm = HF_POISSON_SPECTRAL, B = 3, nx = 128, T = 4, r = 2, S = 3;
};

static int run(const Args &a) {
  const int64_t wb = a.ws_bytes >= 0 ? a.ws_bytes : hf_run_coarse_workspace_bytes(a.B, a.nx, a.T, a.r, a.S);
  return hf_run_coarse(a.st, a.fin, a.plan, a.pm, a.B, a.nx, a.T, a.r, a.S, 0.05f, 5e-3f, 1e-3f, 0.01f, a.traj, a.flux,
                       a.ws, wb, nullptr);
}

static int coarsen(const Args &a) {
  return hf_coarsen_traj(a.traj, a.flux, a.B, a.nx, a.T, a.r, a.S, a.fin, a.flux ? a.st : nullptr, nullptr);
}

int main() {
  const char *fn = "hf_run_coarse", *fc = "hf_coarsen_traj";
  {  // the size query
    EXPECT(hf_run_coarse_workspace_bytes(3, 128, 4, 2, 3) > 0);
    EXPECT(hf_run_coarse_workspace_bytes(3, 128, 1, 2, 3) < hf_run_coarse_workspace_bytes(3, 128, 2, 2, 3));
    // the fine state, 13 fine trajectory rows, 12 fine flux rows (each rounded up to 256 bytes)
    EXPECT(hf_run_coarse_workspace_bytes(3, 128, 4, 2, 3) == 4608 + 13 * 4608 + 18432);
    EXPECT(hf_run_coarse_workspace_bytes(3, 128, 0, 2, 3) == 0);   // T_c = 0: row 0 alone
    EXPECT(hf_run_coarse_workspace_bytes(0, 128, 4, 2, 3) == 0);   // B = 0
    for (int nx : {16, 48, 64, 256, 512, 1024})                     // one launch: no scratch
      EXPECT(hf_run_coarse_workspace_bytes(3, nx, 4, 2, 3) == 0);
    EXPECT(hf_run_coarse_workspace_bytes(32768, 2048, 100000, 64, 16) > 0);  // no int overflow (UBSan)
    EXPECT(hf_run_coarse_workspace_bytes(INT32_MAX, 96, 1, 32, INT32_MAX) == -1);  // more than int64 holds
    EXPECT(hf_run_coarse_workspace_bytes(3, 128, INT32_MAX, 2, 2) == -1);    // T_c * S exceeds int
    EXPECT(hf_run_coarse_workspace_bytes(-1, 128, 4, 2, 3) == -1);
    EXPECT(hf_run_coarse_workspace_bytes(3, 0, 4, 2, 3) == -1);
    EXPECT(hf_run_coarse_workspace_bytes(3, 128, -1, 2, 3) == -1);
    for (int r : {0, -1, 3, 6, 128, INT32_MIN, INT32_MAX}) EXPECT(hf_run_coarse_workspace_bytes(3, 128, 4, r, 3) == -1);
    EXPECT(hf_run_coarse_workspace_bytes(3, 96, 4, 64, 3) == -1);  // r does not divide nx_f
    for (int S : {0, -1, INT32_MIN}) EXPECT(hf_run_coarse_workspace_bytes(3, 128, 4, 2, S) == -1);
  }
  for (int nx : {128, 64, 256}) {  // the sequenced path and both one-launch kernels: the same refusals
    Args a;
    a.nx = nx;
    for (int r : {0, -1, 3, 6, 128, INT32_MIN, INT32_MAX}) {
      Args b = a;
      b.r = r;
      b.ws_bytes = 1 << 20;
      EXPECT(run(b) == HF_EINVAL && named(fn));
      EXPECT(coarsen(b) == HF_EINVAL && named(fc));
    }
    for (int S : {0, -1, INT32_MIN}) {
      Args b = a;
      b.S = S;
      b.ws_bytes = 1 << 20;
      EXPECT(run(b) == HF_EINVAL && named(fn));
      EXPECT(coarsen(b) == HF_EINVAL && named(fc));
    }
    Args b = a;
    b.T = -1, b.ws_bytes = 1 << 20;
    EXPECT(run(b) == HF_EINVAL && named(fn));
    EXPECT(coarsen(b) == HF_EINVAL && named(fc));
    b = a;
    b.B = -1, b.ws_bytes = 1 << 20;
    EXPECT(run(b) == HF_EINVAL && named(fn));
    EXPECT(coarsen(b) == HF_EINVAL && named(fc));
    b = a;
    b.nx = 0, b.ws_bytes = 1 << 20;
    EXPECT(run(b) == HF_EINVAL && named(fn));
    b = a;
    b.fin = nullptr, b.traj = nullptr, b.flux = nullptr;  // no output requested
    EXPECT(run(b) == HF_EINVAL && named(fn));
    b = a;
    b.st = nullptr;
    EXPECT(run(b) == HF_EINVAL && named(fn));
    b = a;
    b.plan = nullptr;
    EXPECT(run(b) == HF_EINVAL && named(fn));
    b = a;
    b.pm = 9;
    EXPECT(run(b) == HF_EINVAL && named(fn));
    b = a;
    b.B = 0;  // nothing to do, before any pointer is looked at
    b.st = nullptr;
    EXPECT(run(b) == HF_OK);
  }
  {  // r must divide nx_f; T_f must be a multiple of S
    Args a;
    a.nx = 96, a.r = 64;
    EXPECT(run(a) == HF_EINVAL && named(fn));
    EXPECT(coarsen(a) == HF_EINVAL && named(fc));
    Args b;
    b.T = 4, b.S = 3;
    EXPECT(coarsen(b) == HF_EINVAL && named(fc));
    b.T = 6;
    b.fin = nullptr;  // NULL coarse trajectory
    EXPECT(coarsen(b) == HF_EINVAL && named(fc));
    Args c;
    c.T = 6;
    EXPECT(hf_coarsen_traj(c.traj, c.flux, c.B, c.nx, c.T, c.r, c.S, c.fin, nullptr, nullptr) == HF_EINVAL && named(fc));
    EXPECT(hf_coarsen_traj(c.traj, nullptr, c.B, c.nx, c.T, c.r, c.S, c.fin, c.st, nullptr) == HF_EINVAL && named(fc));
    EXPECT(hf_coarsen_traj(nullptr, nullptr, 0, c.nx, c.T, c.r, c.S, nullptr, nullptr, nullptr) == HF_OK);
  }
  {  // a workspace too small: one byte short of one coarse step's chunk (the sequenced path only)
    Args a;
    a.ws_bytes = hf_run_coarse_workspace_bytes(a.B, a.nx, 1, a.r, a.S) - 1;
    EXPECT(run(a) == HF_EINVAL && named(fn));
    a.ws_bytes = 0;
    EXPECT(run(a) == HF_EINVAL && named(fn));
  }
  if (hf_device_count() <= 0) {
    // valid arguments: validation passes and the device call fails
    for (int nx : {128, 96, 64, 48, 256, 1024}) {
      Args a;
      a.nx = nx;
      EXPECT(run(a) == HF_EHIP && named(fn));
      a.ws_bytes = hf_run_coarse_workspace_bytes(a.B, a.nx, 1, a.r, a.S);  // chunks of one coarse step
      EXPECT(run(a) == HF_EHIP && named(fn));
      a.T = 0;
      EXPECT(run(a) == HF_EHIP && named(fn));
      Args b;
      b.nx = nx, b.T = 6;
      EXPECT(coarsen(b) == HF_EHIP && named(fc));
    }
    Args a;
    a.pm = HF_POISSON_TRIDIAG;
    EXPECT(run(a) == HF_EHIP && named(fn));
  }
  return finish("coarse_sanitize");
}
