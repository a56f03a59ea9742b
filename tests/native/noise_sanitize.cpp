// Host-sanitized drive of the state-noise entry points of the C ABI
// (hf_gauss_host, hf_state_noise).
//
// Built by `make -C gnn-plasma-flux_amd/csrc asan-noise` with AddressSanitizer
// and UBSan on the HOST code only, like the other programs of this folder.
// hf_gauss_host is host only: it runs the draw code the kernel shares (the
// MT19937 state, its twist and the polar gauss) for odd and even counts, inside
// one 624-word block and across many, into buffers of exactly `count` doubles,
// so a write past the end or an overflow in the integer arithmetic is caught
// here.  hf_state_noise is driven through its validation: every such call must
// be refused before any device call, and the dummy device pointers are never
// dereferenced.  With a device one small call is made (B = 3, nx = 17, zero
// mean, a Poisson plan, node features and the noise output) and its results
// checked for shape-level sanity; without one, valid arguments must fail at the
// launch.  Exit 0 = clean.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "expect.h"

static const int64_t kSeeds[] = {0, 1, 42, 4294967295LL, 1000, 1015};
static const int64_t kCounts[] = {0, 1, 2, 3, 51, 750, 18432};

struct Dev {
  void *p = nullptr;
  explicit Dev(size_t bytes) {
    if (hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) std::abort();
  }
  Dev(const Dev &) = delete;
  ~Dev() { (void)hipFree(p); }
};

static void device_call() {
  const int B = 3, nx = 17;
  std::vector<int64_t> seeds = {42, -1, 1000};  // the middle sample's seed is out of range: NaN rows
  std::vector<float> st(B * 3 * nx), x(nx), out(st.size()), nf(B * nx * 4), noise(st.size());
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < nx; ++i) {
      st[(b * 3 + 0) * nx + i] = 1.0f + 0.1f * std::sin(0.3f * i + b);
      st[(b * 3 + 1) * nx + i] = 0.2f * std::cos(0.3f * i);
      st[(b * 3 + 2) * nx + i] = 0.0f;
    }
  for (int i = 0; i < nx; ++i) x[i] = (i + 0.5f) * 6.2831853f / nx;
  std::vector<double> plan(hf_poisson_plan_len(nx));
  EXPECT(hf_poisson_coeffs(nx, 6.283185307179586, plan.data()) == HF_OK);
  Dev ds(8 * seeds.size()), din(4 * st.size()), dout(4 * st.size()), dpl(8 * plan.size()), dx(4 * x.size()),
      dnf(4 * nf.size()), dnz(4 * noise.size());
  (void)hipMemcpy(ds.p, seeds.data(), 8 * seeds.size(), hipMemcpyHostToDevice);
  (void)hipMemcpy(din.p, st.data(), 4 * st.size(), hipMemcpyHostToDevice);
  (void)hipMemcpy(dpl.p, plan.data(), 8 * plan.size(), hipMemcpyHostToDevice);
  (void)hipMemcpy(dx.p, x.data(), 4 * x.size(), hipMemcpyHostToDevice);
  const float sigma[3] = {1e-2f, 0.0f, 0.0f};
  EXPECT(hf_state_noise((const int64_t *)ds.p, B, nx, sigma, HF_NOISE_ZERO_MEAN, (const float *)din.p, (float *)dout.p,
                        (const double *)dpl.p, HF_POISSON_SPECTRAL, (const float *)dx.p, (float *)dnf.p,
                        (float *)dnz.p, nullptr) == HF_OK);
  EXPECT(hipDeviceSynchronize() == hipSuccess);
  (void)hipMemcpy(out.data(), dout.p, 4 * out.size(), hipMemcpyDeviceToHost);
  (void)hipMemcpy(nf.data(), dnf.p, 4 * nf.size(), hipMemcpyDeviceToHost);
  (void)hipMemcpy(noise.data(), dnz.p, 4 * noise.size(), hipMemcpyDeviceToHost);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < nx; ++i) {
      const float n = out[(b * 3 + 0) * nx + i], u = out[(b * 3 + 1) * nx + i], a = noise[(b * 3 + 0) * nx + i];
      if (b == 1) {
        EXPECT(std::isnan(n) && std::isnan(u));
        continue;
      }
      EXPECT(n == st[(b * 3 + 0) * nx + i] + a && std::fabs(a) < 0.1f && a != 0.0f);
      EXPECT(u == st[(b * 3 + 1) * nx + i] && noise[(b * 3 + 1) * nx + i] == 0.0f);
      EXPECT(nf[(b * nx + i) * 4 + 0] == n && nf[(b * nx + i) * 4 + 2] == out[(b * 3 + 2) * nx + i]);
      EXPECT(nf[(b * nx + i) * 4 + 3] == x[i]);
    }
}

int main() {
  const char *gh = "hf_gauss_host", *sn = "hf_state_noise";
  for (int64_t seed : kSeeds)
    for (int64_t count : kCounts) {
      std::vector<double> g(count, NAN);  // exact size: ASan guards both ends
      EXPECT(hf_gauss_host(seed, count, g.data()) == HF_OK);
      for (double v : g) EXPECT(std::isfinite(v) && std::fabs(v) < 40.0);
    }
  {  // the same seed twice: the same draws; a longer draw starts with the shorter one's pairs
    std::vector<double> a(51), b(51), c(50);
    EXPECT(hf_gauss_host(42, 51, a.data()) == HF_OK && hf_gauss_host(42, 51, b.data()) == HF_OK && a == b);
    EXPECT(hf_gauss_host(42, 50, c.data()) == HF_OK);
    for (int i = 0; i < 50; ++i) EXPECT(a[i] == c[i]);
  }
  {  // refusals of the host entry point
    std::vector<double> g(4);
    for (int64_t seed : {(int64_t)-1, (int64_t)4294967296LL, INT64_MIN, INT64_MAX})
      EXPECT(hf_gauss_host(seed, 4, g.data()) == -1 && named(gh));
    for (int64_t count : {(int64_t)-1, INT64_MIN}) EXPECT(hf_gauss_host(1, count, g.data()) == -1 && named(gh));
    EXPECT(hf_gauss_host(1, INT64_MAX, g.data()) == HF_EUNSUPPORTED && named(gh));
    EXPECT(hf_gauss_host(1, 4, nullptr) == HF_EINVAL && named(gh));
    EXPECT(hf_gauss_host(1, 0, nullptr) == HF_OK);
  }
  {  // hf_state_noise: refused before any device call
    const int64_t *seeds = reinterpret_cast<const int64_t *>(64);
    const float *in = reinterpret_cast<const float *>(128), *x = reinterpret_cast<const float *>(1024);
    float *out = reinterpret_cast<float *>(256), *nf = reinterpret_cast<float *>(2048);
    const double *plan = reinterpret_cast<const double *>(512);
    const float ok[3] = {1e-2f, 1e-2f, 0.0f}, withE[3] = {1e-2f, 0.0f, 5e-3f};
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const int ZM = HF_NOISE_ZERO_MEAN, SP = HF_POISSON_SPECTRAL;
    for (int B : {-1, INT32_MIN})
      EXPECT(hf_state_noise(seeds, B, 64, ok, ZM, in, out, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_EINVAL && named(sn));
    for (int nx : {0, -1, INT32_MIN})
      EXPECT(hf_state_noise(seeds, 3, nx, ok, ZM, in, out, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_EINVAL && named(sn));
    EXPECT(hf_state_noise(nullptr, 3, 64, ok, ZM, in, out, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_EINVAL && named(sn));
    EXPECT(hf_state_noise(seeds, 3, 64, nullptr, ZM, in, out, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_EINVAL && named(sn));
    EXPECT(hf_state_noise(seeds, 3, 64, ok, ZM, nullptr, out, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_EINVAL && named(sn));
    EXPECT(hf_state_noise(seeds, 3, 64, ok, ZM, in, nullptr, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_EINVAL && named(sn));
    for (int ch = 0; ch < 3; ++ch)
      for (float bad : {-1e-2f, nan, -std::numeric_limits<float>::infinity()}) {
        float s[3] = {0.0f, 0.0f, 0.0f};
        s[ch] = bad;
        EXPECT(hf_state_noise(seeds, 3, 64, s, ZM, in, out, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_EINVAL && named(sn));
      }
    for (int flags : {2, 3, -1, INT32_MIN})
      EXPECT(hf_state_noise(seeds, 3, 64, ok, flags, in, out, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_EINVAL && named(sn));
    for (int pm : {2, -1, INT32_MAX})
      EXPECT(hf_state_noise(seeds, 3, 64, ok, ZM, in, out, plan, pm, nullptr, nullptr, nullptr, nullptr) == HF_EINVAL && named(sn));
    EXPECT(hf_state_noise(seeds, 3, 64, withE, ZM, in, out, plan, SP, nullptr, nullptr, nullptr, nullptr) == HF_EINVAL && named(sn));
    EXPECT(hf_state_noise(seeds, 3, 64, ok, ZM, in, out, nullptr, SP, nullptr, nf, nullptr, nullptr) == HF_EINVAL && named(sn));
    EXPECT(hf_state_noise(seeds, 3, 6145, ok, ZM, in, out, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_EUNSUPPORTED && named(sn));
    for (int nx : {(1 << 24) + 1, INT32_MAX})
      EXPECT(hf_state_noise(seeds, 3, nx, ok, 0, in, out, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_EUNSUPPORTED && named(sn));
    EXPECT(hf_state_noise(seeds, 3, 16385, ok, 0, in, out, plan, HF_POISSON_TRIDIAG, nullptr, nullptr, nullptr, nullptr) == HF_EUNSUPPORTED && named(sn));
    EXPECT(hf_state_noise(nullptr, 0, 64, ok, ZM, nullptr, nullptr, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_OK);  // an empty batch
    if (hf_device_count() <= 0) {
      EXPECT(hf_state_noise(seeds, 3, 64, ok, ZM, in, out, plan, SP, x, nf, nullptr, nullptr) == HF_EHIP && named(sn));
      EXPECT(hf_state_noise(seeds, INT32_MAX, 1 << 24, withE, 0, in, out, nullptr, SP, nullptr, nullptr, nullptr, nullptr) == HF_EHIP && named(sn));
    } else {
      device_call();
    }
  }
  return finish("noise_sanitize");
}
