// Host-sanitized drive of the guarded optimizer step's entry points of the C ABI
// (hf_adam_flat_workspace_bytes, hf_adam_flat_ex).
//
// Built by `make -C gnn-plasma-flux_amd/csrc asan-optim` with AddressSanitizer
// and UBSan on the HOST code only, like pinn_unroll_sanitize.cpp.  It walks the
// validation paths: every call in the first part must be refused (or, for an
// empty buffer, accepted) before any device call, so those need no device and
// launch nothing; the dummy device pointers are never dereferenced.  The last
// part hands valid arguments: on a machine without a device the launch itself
// fails and the call returns HF_EHIP (on one with a device the dummy pointers
// would be dereferenced, so that part is skipped there).  Exit 0 = clean.
#include <cmath>
#include <cstdint>

#include "expect.h"

struct Args {
  float *p = reinterpret_cast<float *>(16), *m = reinterpret_cast<float *>(48), *v = reinterpret_cast<float *>(80);
  const float *g = reinterpret_cast<const float *>(32), *dev_lr = nullptr;
  float *step = reinterpret_cast<float *>(112), *stats = nullptr;
  unsigned *done = reinterpret_cast<unsigned *>(128);
  void *ws = reinterpret_cast<void *>(256);
  int64_t n = 10;
  float wd = 0.f, max_norm = INFINITY;
  int skip = 0;
};

static int step(const Args &a) {
  return hf_adam_flat_ex(a.p, a.g, a.m, a.v, a.n, a.step, a.done, a.dev_lr, 1e-3f, 0.9f, 0.999f, 1e-8f, a.wd,
                         a.max_norm, a.skip, a.ws, a.stats, nullptr);
}

int main() {
  const char *fn = "hf_adam_flat_ex";
  // size query: one float64 per workgroup, monotone, capped, no overflow at the largest n (UBSan)
  EXPECT(hf_adam_flat_workspace_bytes(-1) == -1);
  EXPECT(hf_adam_flat_workspace_bytes(INT64_MIN) == -1);
  int64_t last = 0;
  for (int64_t n : {int64_t(0), int64_t(1), int64_t(1024), int64_t(1025), int64_t(230336), int64_t(2048) * 1024,
                    int64_t(2048) * 1024 + 1025, int64_t(1) << 40, INT64_MAX - 1, INT64_MAX}) {
    const int64_t b = hf_adam_flat_workspace_bytes(n);
    EXPECT(b >= 8 && b % 8 == 0 && b >= last && b <= 8 * 2048);
    last = b;
  }
  EXPECT(hf_adam_flat_workspace_bytes(1024) == 8 && hf_adam_flat_workspace_bytes(1025) == 16);
  EXPECT(last == 8 * 2048);

  {  // sizes and required pointers
    Args a;
    for (int64_t n : {int64_t(-1), INT64_MIN}) {
      a.n = n;
      EXPECT(step(a) == HF_EINVAL && named(fn));
    }
    float *Args::*req[] = {&Args::p, &Args::m, &Args::v, &Args::step};
    for (auto q : req) {
      a = Args();
      a.*q = nullptr;
      EXPECT(step(a) == HF_EINVAL && named(fn));
    }
    a = Args();
    a.g = nullptr;
    EXPECT(step(a) == HF_EINVAL && named(fn));
    a = Args();
    a.done = nullptr;
    EXPECT(step(a) == HF_EINVAL && named(fn));
  }
  {  // option values, with and without values to update
    for (int64_t n : {int64_t(10), int64_t(0)}) {
      for (float mn : {0.f, -1.f, -INFINITY, NAN}) {
        Args a;
        a.n = n, a.max_norm = mn;
        EXPECT(step(a) == HF_EINVAL && named(fn));
      }
      for (float wd : {-1e-3f, -INFINITY, NAN}) {
        Args a;
        a.n = n, a.wd = wd;
        EXPECT(step(a) == HF_EINVAL && named(fn));
      }
    }
  }
  {  // the workspace may be missing only when nothing needs the norm
    Args a;
    a.ws = nullptr, a.max_norm = 1.f;
    EXPECT(step(a) == HF_EINVAL && named(fn));
    a = Args();
    a.ws = nullptr, a.skip = 1;
    EXPECT(step(a) == HF_EINVAL && named(fn));
    a = Args();
    a.ws = nullptr, a.stats = reinterpret_cast<float *>(512);
    EXPECT(step(a) == HF_EINVAL && named(fn));
  }
  {  // an empty buffer: HF_OK without a launch, whatever the pointers
    Args a;
    a.n = 0;
    a.p = a.m = a.v = a.step = nullptr, a.g = nullptr, a.done = nullptr, a.ws = nullptr;
    EXPECT(step(a) == HF_OK);
    a = Args();
    a.n = 0, a.max_norm = 1.f, a.wd = 0.1f, a.skip = 1;
    EXPECT(step(a) == HF_OK);
  }
  if (hf_device_count() <= 0) {
    // valid arguments: validation passes and the device call fails -- one launch (no
    // workspace: weight decay alone) and two (the norm's first)
    Args a;
    a.ws = nullptr, a.wd = 0.01f;
    EXPECT(step(a) == HF_EHIP && named(fn));
    a = Args();
    a.max_norm = 1.f, a.skip = 1, a.stats = reinterpret_cast<float *>(512);
    EXPECT(step(a) == HF_EHIP && named(fn));
    a.n = int64_t(2048) * 1024 + 1025;
    EXPECT(step(a) == HF_EHIP && named(fn));
  }
  return finish("optim_sanitize");
}
