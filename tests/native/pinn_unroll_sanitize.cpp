// Host-sanitized drive of PINN's unrolled-training entry points of the C ABI
// (hf_pinn_unroll_workspace_bytes, hf_pinn_unroll_loss, hf_pinn_unroll_adjoint).
//
// Built by `make -C gnn-plasma-flux_amd/csrc asan-pinn-unroll` with
// AddressSanitizer and UBSan on the HOST code only, like
// pure_unroll_sanitize.cpp.  It walks the validation paths: every call in the
// first part must be refused before any device call, so those need no device
// and launch nothing; the dummy device pointers are never dereferenced.  The
// last part hands valid arguments with NULL optional pointers: on a machine
// without a device the launch itself fails and the call returns HF_EHIP (on one
// with a device the dummy pointers would be dereferenced, so that part is
// skipped there).  Exit 0 = clean.
#include <cstdint>

#include "expect.h"

static const float kW[3] = {1.f, 1.f, 1.f};
static const float kLam[3] = {0.1f, 0.1f, 0.01f};

struct Args {
  float *pred = reinterpret_cast<float *>(16), *st = reinterpret_cast<float *>(32), *tg = reinterpret_cast<float *>(48);
  float *next = reinterpret_cast<float *>(80), *carry = reinterpret_cast<float *>(96);
  float *losses = reinterpret_cast<float *>(112), *g = reinterpret_cast<float *>(128);
  double *plan = reinterpret_cast<double *>(160);
  void *ws = reinterpret_cast<void *>(256);
  const float *wp = kW, *phys = kLam;
  int B = 3, nx = 16;
  double dt = 5e-3, dx = 0.1;
  int64_t ws_short = 0;
};

static int loss(const Args &a) {
  const int64_t nb = hf_pinn_unroll_workspace_bytes(a.B < 1 ? 1 : a.B, a.nx < 1 ? 1 : a.nx) - a.ws_short;
  return hf_pinn_unroll_loss(a.pred, a.st, a.tg, a.B, a.nx, a.wp, 1.0f, a.phys, 1.0f, a.dt, a.dx, 1e-3, a.plan,
                             a.losses, a.ws, nb, nullptr);
}
static int adjoint(const Args &a) {
  return hf_pinn_unroll_adjoint(a.pred, a.st, a.tg, a.next, a.carry, a.B, a.nx, a.wp, 1.0f, a.phys, 1.0f, a.dt, a.dx,
                                1e-3, a.plan, a.g, nullptr);
}

// what both entry points refuse alike
template <class F>
static void shared_refusals(F call, const char *fn) {
  float *Args::*req[] = {&Args::pred, &Args::tg};
  for (auto m : req) {
    Args a;
    a.*m = nullptr;
    EXPECT(call(a) == HF_EINVAL && named(fn));
  }
  Args a;
  a.wp = nullptr;
  EXPECT(call(a) == HF_EINVAL && named(fn));
  a = Args();
  a.plan = nullptr;  // phys without its plan
  EXPECT(call(a) == HF_EINVAL && named(fn));
  a = Args();
  a.st = nullptr;  // phys without the state slot
  EXPECT(call(a) == HF_EINVAL && named(fn));
  a = Args();
  a.dt = 0.0;
  EXPECT(call(a) == HF_EINVAL && named(fn));
  a = Args();
  a.dx = -1.0;
  EXPECT(call(a) == HF_EINVAL && named(fn));
  for (int B : {0, -1, INT32_MIN}) {
    a = Args();
    a.B = B;
    EXPECT(call(a) == HF_EINVAL && named(fn));
  }
  for (int nx : {0, -1, INT32_MIN}) {
    a = Args();
    a.nx = nx;
    EXPECT(call(a) == HF_EINVAL && named(fn));
  }
  for (int nx : {6145, INT32_MAX}) {  // beyond the one-workgroup-per-IC LDS plan: unsupported, not invalid
    a = Args();
    a.nx = nx;
    EXPECT(call(a) == HF_EUNSUPPORTED && named(fn));
    a.phys = nullptr, a.st = nullptr, a.plan = nullptr;
    EXPECT(call(a) == HF_EUNSUPPORTED && named(fn));
  }
}

int main() {
  // size query: positive, grows with B, no int overflow at the largest batch (UBSan)
  EXPECT(hf_pinn_unroll_workspace_bytes(3, 16) > 0);
  EXPECT(hf_pinn_unroll_workspace_bytes(1, 1) > 0);
  EXPECT(hf_pinn_unroll_workspace_bytes(32, 64) >= 4 + 32 * 4 * 8);
  EXPECT(hf_pinn_unroll_workspace_bytes(INT32_MAX, 64) > 32LL * INT32_MAX);
  EXPECT(hf_pinn_unroll_workspace_bytes(INT32_MAX, INT32_MAX) > 32LL * INT32_MAX);
  EXPECT(hf_pinn_unroll_workspace_bytes(0, 64) == -1);
  EXPECT(hf_pinn_unroll_workspace_bytes(3, 0) == -1);
  EXPECT(hf_pinn_unroll_workspace_bytes(-5, -5) == -1);
  EXPECT(hf_pinn_unroll_workspace_bytes(INT32_MIN, INT32_MIN) == -1);

  const char *lo = "hf_pinn_unroll_loss", *ad = "hf_pinn_unroll_adjoint";
  shared_refusals(loss, lo);
  shared_refusals(adjoint, ad);
  {  // hf_pinn_unroll_loss: its own outputs and the workspace
    Args a;
    a.losses = nullptr;
    EXPECT(loss(a) == HF_EINVAL && named(lo));
    a = Args();
    a.ws = nullptr;
    EXPECT(loss(a) == HF_EINVAL && named(lo));
    a = Args();
    a.ws_short = 1;
    EXPECT(loss(a) == HF_EINVAL && named(lo));
  }
  {  // hf_pinn_unroll_adjoint: the output, and the output aliasing each input
    Args a;
    a.g = nullptr;
    EXPECT(adjoint(a) == HF_EINVAL && named(ad));
    float *Args::*in[] = {&Args::pred, &Args::st, &Args::tg, &Args::next, &Args::carry};
    for (auto m : in) {
      a = Args();
      a.g = a.*m;
      EXPECT(adjoint(a) == HF_EINVAL && named(ad));
    }
  }
  if (hf_device_count() <= 0) {
    // valid arguments, every optional pointer NULL: validation passes and the device call fails
    Args a;
    a.phys = nullptr, a.st = nullptr, a.plan = nullptr;
    EXPECT(loss(a) == HF_EHIP && named(lo));
    a.next = a.carry = nullptr;
    EXPECT(adjoint(a) == HF_EHIP && named(ad));
  }
  return finish("pinn_unroll_sanitize");
}
