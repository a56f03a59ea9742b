// Host-sanitized drive of PureGNN's unrolled-training entry points of the C ABI
// (hf_pure_unroll_workspace_bytes, hf_pure_unroll_update, hf_pure_unroll_adjoint).
//
// Built by `make -C gnn-plasma-flux_amd/csrc asan-pure-unroll` with
// AddressSanitizer and UBSan on the HOST code only, like unroll_sanitize.cpp.
// It walks the validation paths: every call in the first part must be refused
// with HF_EINVAL before any device call, so those need no device and launch
// nothing; the dummy device pointers are never dereferenced.  The last part
// hands valid arguments with NULL optional pointers: on a machine without a
// device the launch itself fails and the call returns HF_EHIP (on one with a
// device the dummy pointers would be dereferenced, so that part is skipped
// there).  Exit 0 = clean.
#include <cstdint>

#include "expect.h"

static const float kW[3] = {1.f, 1.f, 1.f};

struct Args {
  float *delta = reinterpret_cast<float *>(16), *st = reinterpret_cast<float *>(32), *x = reinterpret_cast<float *>(48);
  float *out = reinterpret_cast<float *>(80), *nf = reinterpret_cast<float *>(96), *tg = reinterpret_cast<float *>(112);
  float *loss = reinterpret_cast<float *>(128), *gdn = reinterpret_cast<float *>(144);
  float *gnf = reinterpret_cast<float *>(160), *gd = reinterpret_cast<float *>(176);
  void *ws = reinterpret_cast<void *>(256);
  const float *wp = kW;
  int B = 3, nx = 16;
  int64_t ws_short = 0;
};

static int update(const Args &a) {
  const int64_t nb = hf_pure_unroll_workspace_bytes(a.B < 1 ? 1 : a.B, a.nx < 1 ? 1 : a.nx) - a.ws_short;
  return hf_pure_unroll_update(a.delta, a.st, a.x, a.B, a.nx, a.out, a.nf, a.tg, a.wp, 1.0f, a.loss, a.ws, nb, nullptr);
}
static int adjoint(const Args &a) {
  return hf_pure_unroll_adjoint(a.out, a.tg, a.wp, 1.0f, a.gdn, a.gnf, a.B, a.nx, a.gd, nullptr);
}

int main() {
  // size query: positive, grows with the tiles, no int overflow at the largest batch (UBSan)
  EXPECT(hf_pure_unroll_workspace_bytes(3, 16) > 0);
  EXPECT(hf_pure_unroll_workspace_bytes(1, 1) > 0);
  EXPECT(hf_pure_unroll_workspace_bytes(4096, 64) >= 4096 * 8);
  EXPECT(hf_pure_unroll_workspace_bytes(3, 10000) >= 3 * 10 * 8);
  EXPECT(hf_pure_unroll_workspace_bytes(0x7fffffff, 1024) > 8LL * 0x7fffffff);
  EXPECT(hf_pure_unroll_workspace_bytes(1, INT32_MAX) > 0);
  EXPECT(hf_pure_unroll_workspace_bytes(0x7fffffff, 1025) == -1);
  EXPECT(hf_pure_unroll_workspace_bytes(INT32_MAX, INT32_MAX) == -1);
  EXPECT(hf_pure_unroll_workspace_bytes(0, 64) == -1);
  EXPECT(hf_pure_unroll_workspace_bytes(3, 0) == -1);
  EXPECT(hf_pure_unroll_workspace_bytes(-5, -5) == -1);
  EXPECT(hf_pure_unroll_workspace_bytes(INT32_MIN, INT32_MIN) == -1);

  const char *up = "hf_pure_unroll_update", *ad = "hf_pure_unroll_adjoint";
  {  // hf_pure_unroll_update: each required pointer, the target's companions, the sizes, the workspace
    float *Args::*req[] = {&Args::delta, &Args::st, &Args::x, &Args::out, &Args::loss};
    for (auto m : req) {
      Args a;
      a.*m = nullptr;
      EXPECT(update(a) == HF_EINVAL && named(up));
    }
    Args a;
    a.ws = nullptr;
    EXPECT(update(a) == HF_EINVAL && named(up));
    a = Args();
    a.wp = nullptr;
    EXPECT(update(a) == HF_EINVAL && named(up));
    a = Args();
    a.out = a.st;
    EXPECT(update(a) == HF_EINVAL && named(up));
    for (int B : {0, -1, INT32_MIN}) {
      a = Args();
      a.B = B;
      EXPECT(update(a) == HF_EINVAL && named(up));
    }
    for (int nx : {0, -1, INT32_MIN}) {
      a = Args();
      a.nx = nx;
      EXPECT(update(a) == HF_EINVAL && named(up));
    }
    a = Args();
    a.ws_short = 1;
    EXPECT(update(a) == HF_EINVAL && named(up));
    a = Args();
    a.B = INT32_MAX, a.nx = INT32_MAX;  // more workgroups than a grid holds
    EXPECT(update(a) == HF_EINVAL && named(up));
  }
  {  // hf_pure_unroll_adjoint
    float *Args::*req[] = {&Args::out, &Args::tg, &Args::gd};
    for (auto m : req) {
      Args a;
      a.*m = nullptr;
      EXPECT(adjoint(a) == HF_EINVAL && named(ad));
    }
    Args a;
    a.wp = nullptr;
    EXPECT(adjoint(a) == HF_EINVAL && named(ad));
    for (int B : {0, -1, INT32_MIN}) {
      a = Args();
      a.B = B;
      EXPECT(adjoint(a) == HF_EINVAL && named(ad));
    }
    for (int nx : {0, -1, INT32_MIN}) {
      a = Args();
      a.nx = nx;
      EXPECT(adjoint(a) == HF_EINVAL && named(ad));
    }
    a = Args();
    a.B = INT32_MAX, a.nx = INT32_MAX;
    EXPECT(adjoint(a) == HF_EINVAL && named(ad));
  }
  if (hf_device_count() <= 0) {
    // valid arguments, every optional pointer NULL: validation passes and the device call fails
    Args a;
    a.nf = a.tg = a.loss = nullptr;
    a.ws = nullptr, a.wp = nullptr;
    EXPECT(update(a) == HF_EHIP && named(up));
    a = Args();
    a.gdn = a.gnf = nullptr;
    EXPECT(adjoint(a) == HF_EHIP && named(ad));
  }
  return finish("pure_unroll_sanitize");
}
