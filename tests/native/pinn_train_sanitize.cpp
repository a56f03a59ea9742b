// Host-sanitized drive of the PINN training entry points of the C ABI
// (hf_pinn_tape_bytes, hf_pinn_backward_workspace_bytes,
// hf_pinn_loss_workspace_bytes, hf_pinn_forward_train, hf_pinn_backward,
// hf_pinn_loss).
//
// Built by `make -C gnn-plasma-flux_amd/csrc asan-pinn-train` with
// AddressSanitizer and UBSan on the HOST code only, like pure_unroll_sanitize.cpp.
// It walks the size queries (extreme arguments included: no integer overflow)
// and the validation paths: every call in the first part must be refused
// before any device call, so those need no device and launch nothing; the dummy
// device pointers are never dereferenced.  The last part hands valid arguments:
// on a machine without a device the launch itself fails and the call returns
// HF_EHIP (on one with a device the dummy pointers would be dereferenced, so
// that part is skipped there).  Exit 0 = clean.
#include <cstdint>

#include "expect.h"

static const float kW[4] = {1.f, 0.1f, 0.1f, 0.01f};

struct Args {
  float *params = reinterpret_cast<float *>(16), *state = reinterpret_cast<float *>(32);
  float *out = reinterpret_cast<float *>(48), *go = reinterpret_cast<float *>(64), *gp = reinterpret_cast<float *>(80);
  float *gs = nullptr, *sn = reinterpret_cast<float *>(96), *losses = reinterpret_cast<float *>(112);
  float *gpred = reinterpret_cast<float *>(128);
  double *plan = reinterpret_cast<double *>(160);
  void *tape = reinterpret_cast<void *>(256), *ws = reinterpret_cast<void *>(512);
  const float *wp = kW;
  int dim = 96, hidden = 64, layers = 3, nx = 32;
  int64_t B = 5;
  double dt = 5e-3, dx = 0.2;
  int64_t ws_short = 0;
};

static int forward(const Args &a) {
  return hf_pinn_forward_train(a.params, a.dim, a.hidden, a.layers, a.state, a.B, a.out, a.tape, nullptr);
}
static int backward(const Args &a) {
  const int64_t nb = hf_pinn_backward_workspace_bytes(96, 64, 3, 5) - a.ws_short;
  return hf_pinn_backward(a.params, a.dim, a.hidden, a.layers, a.state, a.B, a.tape, a.go, a.gp, a.gs, a.ws, nb, nullptr);
}
static int loss(const Args &a) {
  const int64_t nb = hf_pinn_loss_workspace_bytes(5, 32) - a.ws_short;
  return hf_pinn_loss(a.out, a.state, a.sn, (int)a.B, a.nx, a.dt, a.dx, 1e-3, a.wp, a.plan, a.losses, a.gpred, a.ws, nb,
                      nullptr);
}

int main() {
  // size queries: positive, monotone, -1 on bad arguments, no overflow at the extremes (UBSan)
  for (auto fn : {hf_pinn_tape_bytes, hf_pinn_backward_workspace_bytes}) {
    EXPECT(fn(192, 256, 4, 32) > 0);
    EXPECT(fn(3, 8, 2, 1) > 0);
    EXPECT(fn(192, 256, 8, 128000) > fn(192, 256, 4, 128000));
    EXPECT(fn(65536, 65536, 8, 0x7fffffffLL) > 0);
    EXPECT(fn(65537, 256, 4, 32) == -1);
    EXPECT(fn(192, 65537, 4, 32) == -1);
    EXPECT(fn(192, 256, 4, 0x80000000LL) == -1);
    EXPECT(fn(192, 256, 4, INT64_MAX) == -1);
    EXPECT(fn(192, 256, 1, 32) == -1);
    EXPECT(fn(192, 256, 9, 32) == -1);
    EXPECT(fn(192, 256, INT32_MIN, 32) == -1);
    EXPECT(fn(0, 256, 4, 32) == -1);
    EXPECT(fn(192, 0, 4, 32) == -1);
    EXPECT(fn(INT32_MIN, INT32_MIN, 4, 32) == -1);
    EXPECT(fn(192, 256, 4, 0) == -1);
    EXPECT(fn(192, 256, 4, INT64_MIN) == -1);
  }
  EXPECT(hf_pinn_tape_bytes(192, 256, 4, 32) == 3 * 32 * 256 * 4);
  EXPECT(hf_pinn_loss_workspace_bytes(32, 64) >= 32 * 4 * 8);
  EXPECT(hf_pinn_loss_workspace_bytes(1, 1) > 0);
  EXPECT(hf_pinn_loss_workspace_bytes(INT32_MAX, INT32_MAX) > 32LL * INT32_MAX);
  EXPECT(hf_pinn_loss_workspace_bytes(0, 64) == -1);
  EXPECT(hf_pinn_loss_workspace_bytes(32, 0) == -1);
  EXPECT(hf_pinn_loss_workspace_bytes(INT32_MIN, INT32_MIN) == -1);

  const char *fw = "hf_pinn_forward_train", *bw = "hf_pinn_backward", *ls = "hf_pinn_loss";
  {  // the two passes: required pointers, the sizes, the alias, the workspace
    float *Args::*req_f[] = {&Args::params, &Args::state, &Args::out};
    for (auto m : req_f) {
      Args a;
      a.*m = nullptr;
      EXPECT(forward(a) == HF_EINVAL && named(fw));
    }
    float *Args::*req_b[] = {&Args::params, &Args::state, &Args::go, &Args::gp};
    for (auto m : req_b) {
      Args a;
      a.*m = nullptr;
      EXPECT(backward(a) == HF_EINVAL && named(bw));
    }
    Args a;
    a.tape = nullptr;
    EXPECT(forward(a) == HF_EINVAL && named(fw));
    EXPECT(backward(a) == HF_EINVAL && named(bw));
    a = Args();
    a.ws = nullptr;
    EXPECT(backward(a) == HF_EINVAL && named(bw));
    a = Args();
    a.out = a.state;
    EXPECT(forward(a) == HF_EINVAL && named(fw));
    a = Args();
    a.ws_short = 1;
    EXPECT(backward(a) == HF_EINVAL && named(bw));
    for (int64_t B : {(int64_t)0, (int64_t)-1, INT64_MIN}) {
      a = Args();
      a.B = B;
      EXPECT(forward(a) == HF_EINVAL && named(fw));
      EXPECT(backward(a) == HF_EINVAL && named(bw));
    }
    for (int L : {1, 0, 9, INT32_MIN, INT32_MAX}) {
      a = Args();
      a.layers = L;
      EXPECT(forward(a) == HF_EINVAL && named(fw));
      EXPECT(backward(a) == HF_EINVAL && named(bw));
    }
    for (int d : {0, -96, INT32_MIN}) {
      a = Args();
      a.dim = d;
      EXPECT(forward(a) == HF_EINVAL && named(fw));
      EXPECT(backward(a) == HF_EINVAL && named(bw));
      a = Args();
      a.hidden = d;
      EXPECT(forward(a) == HF_EINVAL && named(fw));
      EXPECT(backward(a) == HF_EINVAL && named(bw));
    }
    a = Args();
    a.B = INT64_MAX;
    EXPECT(forward(a) == HF_EUNSUPPORTED && named(fw));
    EXPECT(backward(a) == HF_EUNSUPPORTED && named(bw));
    a = Args();
    a.dim = INT32_MAX;
    EXPECT(forward(a) == HF_EUNSUPPORTED && named(fw));
    EXPECT(backward(a) == HF_EUNSUPPORTED && named(bw));
  }
  {  // hf_pinn_loss
    float *Args::*req[] = {&Args::out, &Args::state, &Args::sn, &Args::losses, &Args::gpred};
    for (auto m : req) {
      Args a;
      a.*m = nullptr;
      EXPECT(loss(a) == HF_EINVAL && named(ls));
    }
    Args a;
    a.wp = nullptr;
    EXPECT(loss(a) == HF_EINVAL && named(ls));
    a = Args();
    a.plan = nullptr;
    EXPECT(loss(a) == HF_EINVAL && named(ls));
    a = Args();
    a.ws = nullptr;
    EXPECT(loss(a) == HF_EINVAL && named(ls));
    a = Args();
    a.ws_short = 1;
    EXPECT(loss(a) == HF_EINVAL && named(ls));
    for (int B : {0, -1, INT32_MIN}) {
      a = Args();
      a.B = B;
      EXPECT(loss(a) == HF_EINVAL && named(ls));
    }
    for (int nx : {0, -1, INT32_MIN}) {
      a = Args();
      a.nx = nx;
      EXPECT(loss(a) == HF_EINVAL && named(ls));
    }
    a = Args();
    a.dt = 0.0;
    EXPECT(loss(a) == HF_EINVAL && named(ls));
    a = Args();
    a.dx = -1.0;
    EXPECT(loss(a) == HF_EINVAL && named(ls));
    for (int nx : {6145, INT32_MAX}) {
      a = Args();
      a.nx = nx;
      EXPECT(loss(a) == HF_EUNSUPPORTED && named(ls));
    }
  }
  if (hf_device_count() <= 0) {
    // valid arguments: validation passes and the device call fails
    Args a;
    EXPECT(forward(a) == HF_EHIP && named(fw));
    EXPECT(backward(a) == HF_EHIP && named(bw));
    EXPECT(loss(a) == HF_EHIP && named(ls));
    a.dim = 15, a.hidden = 16, a.layers = 2;  // the generic path
    EXPECT(forward(a) == HF_EHIP && named(fw));
  }
  return finish("pinn_train_sanitize");
}
