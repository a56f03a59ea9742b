// Host-sanitized drive of the stencil-radius entry points of the C ABI
// (hf_model_create_ex, hf_model_radius, hf_chain_pack_host, hf_graph_flux_radius).
//
// Built by `make -C gnn-plasma-flux_amd/csrc asan-radius` with AddressSanitizer
// and UBSan on the HOST code only, like model_set_sanitize.cpp.  Without a
// device it walks hf_model_create_ex's validation (every bad radius, precision
// or width is refused before any device call) and the host pack at R = 1, 2, 3:
// the stream's update-layer chunks hold W_a unchanged and W_b as float32(w /
// (2R)) in the fragment order capi.cpp documents, the readout chunks do not
// depend on R, and the R = 1 stream is, byte for byte, the one with w * 0.5f
// that hf_model_create has always packed.  With a device it also creates a
// model per radius, checks that nx < 2R + 1 is refused, and that a radius-1
// model of hf_model_create_ex steps like hf_model_create's.  Exit 0 = clean.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "expect.h"

static const int kH = 128, kIn = 4;

static std::vector<float> params(int layers, unsigned seed) {
  std::vector<float> p((size_t)hf_model_param_count(kIn, kH, layers));
  for (float &v : p) {
    seed = seed * 1664525u + 1013904223u;
    v = 0.05f * (((seed >> 8) & 0xFFFF) / 65536.0f - 0.5f);
  }
  return p;
}

static void validation() {
  const std::vector<float> p = params(1, 7);
  hf_model_t m = reinterpret_cast<hf_model_t>(8);
  for (int radius : {0, 4, -1, 1 << 30}) {
    EXPECT(hf_model_create_ex(p.data(), kIn, kH, 1, HF_WDTYPE_F32, radius, &m) == HF_EINVAL && named("radius"));
    EXPECT(m == nullptr);
  }
  for (int wd : {HF_WDTYPE_BF16, HF_WDTYPE_F16X3})
    for (int radius : {2, 3})
      EXPECT(hf_model_create_ex(p.data(), kIn, kH, 1, wd, radius, &m) == HF_EUNSUPPORTED && named("float32"));
  const std::vector<float> narrow((size_t)hf_model_param_count(kIn, 64, 1), 0.01f);
  EXPECT(hf_model_create_ex(narrow.data(), kIn, 64, 1, HF_WDTYPE_F32, 2, &m) == HF_EUNSUPPORTED);
  EXPECT(hf_model_create_ex(nullptr, kIn, kH, 1, HF_WDTYPE_F32, 2, &m) == HF_EINVAL);
  EXPECT(hf_model_create_ex(p.data(), kIn, kH, 1, HF_WDTYPE_F32, 2, nullptr) == HF_EINVAL);
  EXPECT(hf_model_create_ex(p.data(), kIn, kH, 1, 9, 2, &m) == HF_EINVAL);
  EXPECT(hf_model_create_ex(p.data(), 0, kH, 1, HF_WDTYPE_F32, 2, &m) == HF_EINVAL);
  EXPECT(hf_model_radius(nullptr) == 0);
  EXPECT(hf_graph_flux_radius(nullptr, nullptr, 1, 7, nullptr, nullptr, nullptr, nullptr) == HF_EINVAL &&
         named("hf_graph_flux_radius"));
  // the pack's own refusals
  EXPECT(hf_chain_pack_host(p.data(), 1, HF_WDTYPE_F32, 0, nullptr, 0) == -1);
  EXPECT(hf_chain_pack_host(p.data(), 1, HF_WDTYPE_F32, 4, nullptr, 0) == -1);
  EXPECT(hf_chain_pack_host(p.data(), 9, HF_WDTYPE_F32, 1, nullptr, 0) == -1);
  EXPECT(hf_chain_pack_host(p.data(), -1, HF_WDTYPE_F32, 1, nullptr, 0) == -1);
  EXPECT(hf_chain_pack_host(p.data(), 1, HF_WDTYPE_BF16, 2, nullptr, 0) == -1);
  EXPECT(hf_chain_pack_host(p.data(), 1, 7, 1, nullptr, 0) == -1);
  std::vector<float> small(16);
  EXPECT(hf_chain_pack_host(p.data(), 1, HF_WDTYPE_F32, 1, small.data(), 64) == -1);
  EXPECT(hf_chain_pack_host(nullptr, 1, HF_WDTYPE_F32, 1, small.data(), 1 << 30) == -1);
  EXPECT(hf_chain_pack_host(p.data(), 1, HF_WDTYPE_BF16, 1, nullptr, 0) == (8 + 8) * 8192 + 8192);
  EXPECT(hf_chain_pack_host(p.data(), 1, HF_WDTYPE_F16X3, 1, nullptr, 0) == (8 + 8) * 16384);
}

// k of k-step s, lane (capi.cpp kperm)
static int kperm(int s, int lane) { return 16 * (s >> 2) + 4 * (lane >> 4) + (s & 3); }

static std::vector<float> pack(const std::vector<float> &p, int layers, int radius) {
  const int64_t bytes = hf_chain_pack_host(p.data(), layers, HF_WDTYPE_F32, radius, nullptr, 0);
  EXPECT(bytes == (int64_t)(16 * layers + 16) * 8192);
  std::vector<float> out((size_t)(bytes > 0 ? bytes / 4 : 0));
  EXPECT(hf_chain_pack_host(p.data(), layers, HF_WDTYPE_F32, radius, out.data(), bytes) == bytes);
  return out;
}

static void packs(int layers) {
  const std::vector<float> p = params(layers, 100 + layers);
  const int64_t per_layer = (int64_t)kH * 2 * kH + kH, w_l = (int64_t)kH * kIn + kH;
  std::vector<float> by_radius[4];
  for (int R = 1; R <= 3; ++R) {
    const std::vector<float> &st = by_radius[R] = pack(p, layers, R);
    if (st.empty()) continue;
    int bad = 0;
    for (int c = 0; c < 16 * layers; ++c)  // update-layer chunk (l, gi): [j 8][lane 64][4]
      for (int j = 0; j < 8; ++j)
        for (int lane = 0; lane < 64; ++lane)
          for (int cc = 0; cc < 4; ++cc) {
            const int l = c / 16, s = 4 * (c % 16) + (j >> 1), nt = 4 * (j & 1) + cc;
            const int k = (s < 32 ? 0 : kH) + kperm(s % 32, lane);
            const float w = p[(size_t)(w_l + l * per_layer + (int64_t)(16 * nt + (lane & 15)) * 2 * kH + k)];
            const float want = s < 32 ? w : w / (float)(2 * R);
            const float got = st[(size_t)(((c * 8 + j) * 64 + lane) * 4 + cc)];
            bad += std::memcmp(&got, &want, 4) != 0;
            if (R == 1 && s >= 32) {  // what hf_model_create packed before the radius existed
              const float half = w * 0.5f;
              bad += std::memcmp(&got, &half, 4) != 0;
            }
          }
    EXPECT(bad == 0);
  }
  // the readout chunks do not know the radius
  const size_t ro = (size_t)16 * layers * 2048;
  for (int R = 2; R <= 3; ++R)
    if (by_radius[R].size() == by_radius[1].size() && by_radius[1].size() >= ro)
      EXPECT(std::memcmp(by_radius[R].data() + ro, by_radius[1].data() + ro, (by_radius[1].size() - ro) * 4) == 0);
  if (layers > 0) EXPECT(by_radius[1] != by_radius[2] && by_radius[2] != by_radius[3]);
}

struct Dev {
  void *p = nullptr;
  explicit Dev(size_t bytes) {
    if (hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) std::abort();
    (void)hipMemset(p, 0, bytes ? bytes : 4);
  }
  ~Dev() { (void)hipFree(p); }
  float *f() const { return static_cast<float *>(p); }
  double *d() const { return static_cast<double *>(p); }
};

static void device() {
  const int layers = 2, nx = 64, B = 5;
  const std::vector<float> p = params(layers, 31);
  hf_model_t plain = nullptr, m[4] = {nullptr, nullptr, nullptr, nullptr};
  EXPECT(hf_model_create(p.data(), kIn, kH, layers, HF_WDTYPE_F32, &plain) == HF_OK && hf_model_radius(plain) == 1);
  for (int R = 1; R <= 3; ++R)
    EXPECT(hf_model_create_ex(p.data(), kIn, kH, layers, HF_WDTYPE_F32, R, &m[R]) == HF_OK && hf_model_radius(m[R]) == R);
  const double L = 2 * M_PI, dx = L / nx;
  const float c = (float)(5e-3 / dx), dt = 5e-3f, nu = 1e-3f, dx2 = (float)(dx * dx);
  std::vector<float> h((size_t)B * 3 * nx), x((size_t)nx);
  for (int i = 0; i < nx; ++i) x[i] = (float)((i + 0.5) * dx);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < nx; ++i) {
      h[(size_t)(b * 3 * nx + i)] = 1.f + 0.01f * std::sin((b % 3 + 1) * x[i]);
      h[(size_t)(b * 3 * nx + nx + i)] = 0.01f * std::cos((b % 5 + 2) * x[i]);
      h[(size_t)(b * 3 * nx + 2 * nx + i)] = 0.f;
    }
  std::vector<double> plan((size_t)hf_poisson_plan_len(nx));
  EXPECT(hf_poisson_coeffs(nx, L, plan.data()) == HF_OK);
  Dev st(4 * h.size()), dx_(4 * x.size()), pc(8 * plan.size());
  (void)hipMemcpy(st.p, h.data(), 4 * h.size(), hipMemcpyHostToDevice);
  (void)hipMemcpy(dx_.p, x.data(), 4 * x.size(), hipMemcpyHostToDevice);
  (void)hipMemcpy(pc.p, plan.data(), 8 * plan.size(), hipMemcpyHostToDevice);
  std::vector<float> fin[4];
  hf_model_t all[4] = {plain, m[1], m[2], m[3]};
  for (int i = 0; i < 4; ++i) {
    Dev out(4 * h.size());
    fin[i].resize(h.size());
    if (!all[i]) continue;
    EXPECT(hf_run(all[i], st.f(), out.f(), dx_.f(), pc.d(), B, nx, 3, c, dt, nu, dx2, nullptr, nullptr, nullptr, nullptr,
                  0, nullptr) == HF_OK);
    EXPECT(hipDeviceSynchronize() == hipSuccess);
    (void)hipMemcpy(fin[i].data(), out.p, 4 * h.size(), hipMemcpyDeviceToHost);
  }
  EXPECT(fin[0] == fin[1]);                      // radius 1 of the new call is hf_model_create
  EXPECT(fin[1] != fin[2] && fin[2] != fin[3]);  // the radius reaches the kernels
  // nx < 2R + 1 is refused by every entry point before a launch (the pointers are not read)
  Dev out(4 * h.size());
  if (m[3]) {
    EXPECT(hf_run(m[3], st.f(), out.f(), dx_.f(), pc.d(), B, 6, 3, c, dt, nu, dx2, nullptr, nullptr, nullptr, nullptr, 0,
                  nullptr) == HF_EINVAL && named("hf_run"));
    EXPECT(hf_step(m[3], st.f(), out.f(), dx_.f(), pc.d(), B, 6, c, dt, nu, dx2, nullptr, nullptr, nullptr, 0,
                   nullptr) == HF_EINVAL && named("hf_step"));
    EXPECT(hf_chain_flux(m[3], st.f(), 2, 6, out.f(), nullptr, nullptr) == HF_EINVAL && named("hf_chain_flux"));
    EXPECT(hf_graph_flux_radius(m[3], st.f(), 2, 6, nullptr, out.f(), out.f(), nullptr) == HF_EINVAL);
    EXPECT(hf_graph_flux_radius(m[3], st.f(), -1, 7, nullptr, out.f(), out.f(), nullptr) == HF_EINVAL);
    EXPECT(hf_graph_flux_radius(m[3], st.f(), 2, 7, nullptr, out.f(), out.f(), nullptr) == HF_EINVAL);  // NULL edges
    EXPECT(hf_graph_flux_radius(m[3], st.f(), 0, 7, nullptr, nullptr, nullptr, nullptr) == HF_OK);
  }
  if (m[2] && m[3]) {
    hf_model_t mixed[2] = {m[2], m[3]};
    hf_model_set_t set = nullptr;
    EXPECT(hf_model_set_create(mixed, 2, &set) == HF_EUNSUPPORTED && set == nullptr);
    hf_model_t equal[2] = {m[2], m[2]};
    EXPECT(hf_model_set_create(equal, 2, &set) == HF_OK && hf_model_set_size(set) == 2);
    hf_model_set_destroy(set);
  }
  for (hf_model_t q : all) hf_model_destroy(q);
  std::printf("device checks done\n");
}

int main() {
  validation();
  for (int layers : {0, 1, 4, 8}) packs(layers);
  const int ndev = hf_device_count();
  std::printf("validation and packs done (%d failures); devices: %d; %s\n", g_fail, ndev, hf_version());
  if (ndev > 0) device();
  return finish("radius_sanitize");
}
