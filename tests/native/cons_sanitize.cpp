// Host-sanitized drive of the conservation-term entry points of the C ABI
// (hf_state_moments, hf_unroll_update_ex / hf_unroll_adjoint_ex,
// hf_pure_unroll_update_ex / hf_pure_unroll_adjoint_ex, hf_pinn_unroll_loss_ex /
// hf_pinn_unroll_adjoint_ex and the three hf_*_workspace_bytes_ex queries).
//
// Built by `make -C gnn-plasma-flux_amd/csrc asan-cons` with AddressSanitizer
// and UBSan on the HOST code only, like unroll_sanitize.cpp.  It walks the
// validation paths: every call in the first part must be refused with HF_EINVAL
// before any device call, so those need no device and launch nothing; the dummy
// device pointers are never dereferenced.  The last part hands valid arguments
// with NULL optional pointers: on a machine without a device the launch itself
// fails and the call returns HF_EHIP (on one with a device the dummy pointers
// would be dereferenced, so that part is skipped there).  Exit 0 = clean.
#include <cmath>
#include <cstdint>

#include "expect.h"

static const float kW[3] = {1.f, 1.f, 1.f};
static const float kLam[2] = {1.f, 0.5f};

static float *fp(uintptr_t v) { return reinterpret_cast<float *>(v); }

struct Args {
  float *in = fp(16), *st = fp(32), *x = fp(48), *out = fp(80), *nf = fp(96), *tg = fp(112), *losses = fp(128);
  float *coef = fp(144), *g = fp(160);
  double *plan = reinterpret_cast<double *>(192), *ref = reinterpret_cast<double *>(224);
  void *ws = reinterpret_cast<void *>(256);
  const float *wp = kW, *cons = kLam;
  int B = 3, nx = 16;
  int64_t ws_short = 0;
};

typedef int (*Call)(const Args &);
typedef int64_t (*Query)(int, int);

static int64_t bytes(Query q, const Args &a) { return q(a.B < 1 ? 1 : a.B, a.nx < 1 ? 1 : a.nx) - a.ws_short; }

static int hybrid(const Args &a) {
  return hf_unroll_update_ex(a.in, a.st, a.x, a.plan, HF_POISSON_SPECTRAL, a.B, a.nx, 0.1f, 0.1f, a.out, a.nf, a.tg, a.wp,
                             1.0f, a.losses, a.ws, bytes(hf_unroll_workspace_bytes_ex, a), a.cons, 1.0f, a.ref, a.coef,
                             nullptr);
}
static int pure(const Args &a) {
  return hf_pure_unroll_update_ex(a.in, a.st, a.x, a.B, a.nx, a.out, a.nf, a.tg, a.wp, 1.0f, a.losses, a.ws,
                                  bytes(hf_pure_unroll_workspace_bytes_ex, a), a.cons, 1.0f, a.ref, a.coef, nullptr);
}
static int pinn(const Args &a) {
  return hf_pinn_unroll_loss_ex(a.in, nullptr, a.tg, a.B, a.nx, a.wp, 1.0f, nullptr, 0.f, 0.0, 0.0, 0.0, nullptr,
                                a.losses, a.ws, bytes(hf_pinn_unroll_workspace_bytes_ex, a), a.cons, 1.0f, a.ref, a.coef,
                                nullptr);
}
static int hybrid_adj(const Args &a) {
  return hf_unroll_adjoint_ex(a.st, a.out, a.tg, a.wp, 1.0f, nullptr, nullptr, a.plan, HF_POISSON_SPECTRAL, a.B, a.nx,
                              0.1f, 0.1f, a.g, nullptr, a.coef, nullptr);
}
static int pure_adj(const Args &a) {
  return hf_pure_unroll_adjoint_ex(a.out, a.tg, a.wp, 1.0f, nullptr, nullptr, a.B, a.nx, a.g, a.coef, nullptr);
}
static int pinn_adj(const Args &a) {
  return hf_pinn_unroll_adjoint_ex(a.in, nullptr, a.tg, nullptr, nullptr, a.B, a.nx, a.wp, 1.0f, nullptr, 0.f, 0.0, 0.0,
                                   0.0, nullptr, a.g, a.coef, nullptr);
}

int main() {
  {  // hf_state_moments
    const char *fn = "hf_state_moments";
    double *m = reinterpret_cast<double *>(64);
    EXPECT(hf_state_moments(nullptr, 3, 16, m, nullptr) == HF_EINVAL && named(fn));
    EXPECT(hf_state_moments(fp(16), 3, 16, nullptr, nullptr) == HF_EINVAL && named(fn));
    for (int64_t rows : {(int64_t)0, (int64_t)-1, INT64_MIN, INT64_MAX, (int64_t)1 << 34})
      EXPECT(hf_state_moments(fp(16), rows, 16, m, nullptr) == HF_EINVAL && named(fn));
    for (int nx : {0, -1, INT32_MIN}) EXPECT(hf_state_moments(fp(16), 3, nx, m, nullptr) == HF_EINVAL && named(fn));
  }
  struct Fwd {
    const char *name;
    Call call;
    Query plain, ex;
    int per_ic;
  } fwd[] = {{"hf_unroll_update_ex", hybrid, hf_unroll_workspace_bytes, hf_unroll_workspace_bytes_ex, 2},
             {"hf_pure_unroll_update_ex", pure, hf_pure_unroll_workspace_bytes, hf_pure_unroll_workspace_bytes_ex, 3},
             {"hf_pinn_unroll_loss_ex", pinn, hf_pinn_unroll_workspace_bytes, hf_pinn_unroll_workspace_bytes_ex, 2}};
  for (const Fwd &f : fwd) {
    // size query: the plain size and the terms' partials, no int overflow at the largest batch (UBSan)
    EXPECT(f.ex(3, 16) >= f.plain(3, 16) + f.per_ic * 8 * 3);
    EXPECT(f.ex(1, 1) > f.plain(1, 1));
    EXPECT(f.ex(0x7fffffff, 1024) > 8LL * (1 + f.per_ic) * 0x7fffffff);
    EXPECT(f.ex(0, 64) == -1 && f.ex(3, 0) == -1 && f.ex(-5, -5) == -1 && f.ex(INT32_MIN, INT32_MIN) == -1);
    // cons without what it needs
    {
      Args a;
      a.ref = nullptr;
      EXPECT(f.call(a) == HF_EINVAL && named(f.name));
      a = Args();
      a.coef = nullptr;
      EXPECT(f.call(a) == HF_EINVAL && named(f.name));
      a = Args();
      a.ws = nullptr;
      EXPECT(f.call(a) == HF_EINVAL && named(f.name));
      a = Args();
      a.tg = nullptr;
      EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    }
    // a lam that is negative or NaN
    for (int j = 0; j < 2; ++j)
      for (float bad : {-1.f, -1e-30f, NAN, -INFINITY}) {
        float lam[2] = {1.f, 1.f};
        lam[j] = bad;
        Args a;
        a.cons = lam;
        EXPECT(f.call(a) == HF_EINVAL && named(f.name));
      }
    // a workspace too small: one byte short, and the plain size with cons
    Args a;
    a.ws_short = 1;
    EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    a.ws_short = f.ex(3, 16) - f.plain(3, 16);
    EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    a.cons = nullptr, a.ref = nullptr, a.coef = nullptr;
    a.ws_short += 1;  // and below the plain size without cons
    EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    // the buffers without cons
    a = Args();
    a.cons = nullptr, a.coef = nullptr;
    EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    a = Args();
    a.cons = nullptr, a.ref = nullptr;
    EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    // required pointers and sizes, as the plain calls
    float *Args::*req[] = {&Args::in, &Args::losses};
    for (auto m : req) {
      a = Args();
      a.*m = nullptr;
      EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    }
    a = Args();
    a.wp = nullptr;
    EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    for (int v : {0, -1, INT32_MIN}) {
      a = Args();
      a.B = v;
      EXPECT(f.call(a) == HF_EINVAL && named(f.name));
      a = Args();
      a.nx = v;
      EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    }
  }
  {  // the nx limits are unchanged
    Args a;
    a.nx = 6145;
    EXPECT(hybrid(a) == HF_EUNSUPPORTED && pinn(a) == HF_EUNSUPPORTED);
    EXPECT(hybrid_adj(a) == HF_EUNSUPPORTED && pinn_adj(a) == HF_EUNSUPPORTED);
    a.B = INT32_MAX, a.nx = INT32_MAX;  // more workgroups than a grid holds
    EXPECT(pure(a) == HF_EINVAL && pure_adj(a) == HF_EINVAL);
  }
  struct Adj {
    const char *name;
    Call call;
  } adj[] = {{"hf_unroll_adjoint_ex", hybrid_adj}, {"hf_pure_unroll_adjoint_ex", pure_adj},
             {"hf_pinn_unroll_adjoint_ex", pinn_adj}};
  for (const Adj &f : adj) {
    float *Args::*req[] = {&Args::tg, &Args::g};
    for (auto m : req) {
      Args a;
      a.*m = nullptr;
      EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    }
    Args a;
    a.wp = nullptr;
    EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    for (int v : {0, -1, INT32_MIN}) {
      a = Args();
      a.B = v;
      EXPECT(f.call(a) == HF_EINVAL && named(f.name));
      a = Args();
      a.nx = v;
      EXPECT(f.call(a) == HF_EINVAL && named(f.name));
    }
  }
  {
    Args a;
    a.coef = a.g;  // PINN's gradient is written while the coefficients are still read
    EXPECT(pinn_adj(a) == HF_EINVAL && named("hf_pinn_unroll_adjoint_ex"));
  }
  if (hf_device_count() <= 0) {
    // valid arguments: validation passes and the device call fails
    Args a;
    EXPECT(hf_state_moments(a.st, 3, 16, a.ref, nullptr) == HF_EHIP && named("hf_state_moments"));
    for (const Fwd &f : fwd) {
      EXPECT(f.call(a) == HF_EHIP && named(f.name));
      Args b;
      b.cons = nullptr, b.ref = nullptr, b.coef = nullptr;
      EXPECT(f.call(b) == HF_EHIP && named(f.name));
    }
    for (const Adj &f : adj) {
      EXPECT(f.call(a) == HF_EHIP && named(f.name));
      Args b;
      b.coef = nullptr;
      EXPECT(f.call(b) == HF_EHIP && named(f.name));
    }
  }
  return finish("cons_sanitize");
}
