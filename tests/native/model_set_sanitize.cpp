// Host-sanitized drive of the model-set entry points of the C ABI
// (hf_model_set_create / _destroy / _size, hf_run_set, hf_run_compare_set,
// hf_set_workspace_need).
//
// Built by `make -C gnn-plasma-flux_amd/csrc asan-model-set` with
// AddressSanitizer and UBSan on the HOST code only, like score_sanitize.cpp.
// Without a device it walks the validation paths: every call must be refused
// before any device call, so the dummy device pointers are never
// dereferenced.  With a device it also rolls a set of M = 2 models (2 and 4
// layers) out at a tiny size, fused (nx 64) and model after model (nx 20),
// shared and per-model ICs, and checks that model m's block equals the
// single-model call's, bit for bit.  Exit 0 = clean.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "expect.h"

static float *const kS0 = reinterpret_cast<float *>(32), *const kFin = reinterpret_cast<float *>(48);
static float *const kX = reinterpret_cast<float *>(64), *const kMse = reinterpret_cast<float *>(128);
static double *const kPlan = reinterpret_cast<double *>(80);

static int run(hf_model_set_t set, const float *s0, int64_t stride, float *fin, int B, int nx, int T,
               int pm = HF_POISSON_SPECTRAL) {
  return hf_run_set(set, s0, stride, fin, kX, kPlan, pm, B, nx, T, 0.05f, 5e-3f, 1e-3f, 0.01f, nullptr, nullptr, nullptr,
                    nullptr, 0, nullptr);
}
static int compare(hf_model_set_t set, const float *s0, int64_t stride, float *fin, int B, int nx, int T,
                   int pm = HF_POISSON_SPECTRAL) {
  return hf_run_compare_set(set, s0, stride, fin, kX, kPlan, pm, B, nx, T, 0.05f, 5e-3f, 1e-3f, 0.01f, kMse, nullptr,
                            nullptr, nullptr, 0, nullptr);
}

static void validation() {
  hf_model_set_t set = reinterpret_cast<hf_model_set_t>(8);
  hf_model_t none[2] = {nullptr, nullptr};
  EXPECT(hf_model_set_create(nullptr, 2, &set) == HF_EINVAL && named("hf_model_set_create") && set == nullptr);
  EXPECT(hf_model_set_create(none, 2, nullptr) == HF_EINVAL && named("hf_model_set_create"));
  EXPECT(hf_model_set_create(none, 0, &set) == HF_EINVAL && named("hf_model_set_create"));
  EXPECT(hf_model_set_create(none, -3, &set) == HF_EINVAL && named("hf_model_set_create"));
  EXPECT(hf_model_set_create(none, 2, &set) == HF_EINVAL && named("hf_model_set_create") && set == nullptr);
  hf_model_set_destroy(nullptr);
  EXPECT(hf_model_set_size(nullptr) == 0);
  EXPECT(hf_set_workspace_need(nullptr, HF_OP_RUN, 3, 64, 5, 0) == -1);
  for (auto call : {run, compare}) {
    const char *fn = call == run ? "hf_run_set" : "hf_run_compare_set";
    EXPECT(call(nullptr, kS0, 0, kFin, 3, 64, 5, 0) == HF_EINVAL && named(fn));             // NULL set
    EXPECT(call(nullptr, kS0, 0, kFin, -1, 64, 5, 0) == HF_EINVAL && named(fn));
    EXPECT(call(nullptr, kS0, 0, kFin, 3, 0, 5, 0) == HF_EINVAL && named(fn));
    EXPECT(call(nullptr, kS0, 0, kFin, 3, 64, -1, 0) == HF_EINVAL && named(fn));
    EXPECT(call(nullptr, kS0, 1, kFin, 3, 64, 5, 0) == HF_EINVAL && named("model_stride"));  // neither 0 nor B*3*nx
    EXPECT(call(nullptr, kS0, 3 * 3 * 64 - 1, kFin, 3, 64, 5, 0) == HF_EINVAL && named("model_stride"));
    EXPECT(call(nullptr, kS0, -3 * 3 * 64, kFin, 3, 64, 5, 0) == HF_EINVAL && named("model_stride"));
    EXPECT(call(nullptr, kS0, 1, kFin, INT32_MAX, INT32_MAX, 5, 0) == HF_EINVAL &&
           named("model_stride"));  // B*3*nx is past 2^63 here: no int overflow (UBSan)
    EXPECT(call(nullptr, kS0, 0, kS0, 3, 64, 5, 0) == HF_EINVAL && named("alias"));           // shared ICs in place
    EXPECT(call(nullptr, kS0, 3 * 3 * 64, kS0, 3, 64, 5, 0) == HF_EINVAL && named("NULL model set"));
  }
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

static std::vector<float> host(const Dev &d, size_t n) {
  std::vector<float> v(n);
  (void)hipMemcpy(v.data(), d.p, 4 * n, hipMemcpyDeviceToHost);
  return v;
}

// the set's rollouts at B ICs x nx cells against one call per model
static void rollouts(hf_model_set_t set, hf_model_t *models, int M, int B, int nx, int T) {
  const int64_t S = 3LL * nx, MS = B * S;
  const double L = 2 * M_PI, dx = L / nx;
  const float c = (float)(5e-3 / dx), dt = 5e-3f, nu = 1e-3f, dx2 = (float)(dx * dx);
  std::vector<float> h((size_t)(M * MS)), x((size_t)nx);
  for (int i = 0; i < nx; ++i) x[i] = (float)((i + 0.5) * dx);
  for (int b = 0; b < M * B; ++b)
    for (int i = 0; i < nx; ++i) {
      h[b * S + i] = 1.f + 0.01f * std::sin((b % 3 + 1) * x[i]);
      h[b * S + nx + i] = 0.01f * std::cos((b % 5 + 2) * x[i]);
      h[b * S + 2 * nx + i] = 0.f;
    }
  std::vector<double> plan((size_t)hf_poisson_plan_len(nx));
  EXPECT(hf_poisson_coeffs(nx, L, plan.data()) == HF_OK);
  const size_t nfin = (size_t)(M * MS), nser = (size_t)M * B * (T + 1);
  Dev st(4 * h.size()), fin(4 * nfin), one(4 * nfin), dx_(4 * x.size()), pc(8 * plan.size());
  Dev traj(4 * nser * S), flux(4 * (size_t)M * B * T * nx), met(16 * nser), mcl(16 * nser), mse(12 * nser);
  Dev mse1(12 * nser);
  (void)hipMemcpy(st.p, h.data(), 4 * h.size(), hipMemcpyHostToDevice);
  (void)hipMemcpy(dx_.p, x.data(), 4 * x.size(), hipMemcpyHostToDevice);
  (void)hipMemcpy(pc.p, plan.data(), 8 * plan.size(), hipMemcpyHostToDevice);
  EXPECT(hf_poisson(st.f(), (int)S, st.f() + 2 * nx, (int)S, pc.d(), M * B, nx, nullptr) == HF_OK);
  EXPECT(hf_set_workspace_need(set, HF_OP_RUN, B, nx, T, HF_WS_TRAJ) >= 0);
  EXPECT(hf_set_workspace_need(set, HF_OP_STEP, B, nx, T, 0) == -1);
  for (int64_t stride : {(int64_t)0, MS}) {
    EXPECT(hf_run_set(set, st.f(), stride, fin.f(), dx_.f(), pc.d(), HF_POISSON_SPECTRAL, B, nx, T, c, dt, nu, dx2,
                      traj.f(), flux.f(), met.f(), nullptr, 0, nullptr) == HF_OK);
    for (int m = 0; m < M; ++m)
      EXPECT(hf_run(models[m], st.f() + m * stride, one.f() + m * MS, dx_.f(), pc.d(), B, nx, T, c, dt, nu, dx2, nullptr,
                    nullptr, nullptr, nullptr, 0, nullptr) == HF_OK);
    EXPECT(hipDeviceSynchronize() == hipSuccess);
    EXPECT(host(fin, nfin) == host(one, nfin));
    EXPECT(hf_run_compare_set(set, st.f(), stride, fin.f(), dx_.f(), pc.d(), HF_POISSON_SPECTRAL, B, nx, T, c, dt, nu,
                              dx2, mse.f(), met.f(), mcl.f(), nullptr, 0, nullptr) == HF_OK);
    for (int m = 0; m < M; ++m)
      EXPECT(hf_run_compare(models[m], st.f() + m * stride, one.f() + m * MS, dx_.f(), pc.d(), B, nx, T, c, dt, nu, dx2,
                            mse1.f() + (size_t)m * B * (T + 1) * 3, nullptr, nullptr, nullptr, 0, nullptr) == HF_OK);
    EXPECT(hipDeviceSynchronize() == hipSuccess);
    EXPECT(host(fin, nfin) == host(one, nfin));
    EXPECT(host(mse, 3 * nser) == host(mse1, 3 * nser));
  }
  // the refusals that need a real set
  EXPECT(hf_run_set(set, st.f(), 7, fin.f(), dx_.f(), pc.d(), 0, B, nx, T, c, dt, nu, dx2, nullptr, nullptr, nullptr,
                    nullptr, 0, nullptr) == HF_EINVAL);
  EXPECT(hf_run_set(set, st.f(), 0, st.f(), dx_.f(), pc.d(), 0, B, nx, T, c, dt, nu, dx2, nullptr, nullptr, nullptr,
                    nullptr, 0, nullptr) == HF_EINVAL);
  EXPECT(hf_run_set(set, st.f(), 0, fin.f(), dx_.f(), pc.d(), 9, B, nx, T, c, dt, nu, dx2, nullptr, nullptr, nullptr,
                    nullptr, 0, nullptr) != HF_OK);
  EXPECT(hf_run_compare_set(set, st.f(), 0, fin.f(), dx_.f(), pc.d(), 0, B, nx, T, c, dt, nu, dx2, nullptr, nullptr,
                            nullptr, nullptr, 0, nullptr) == HF_EINVAL);
}

int main() {
  validation();
  const int ndev = hf_device_count();
  std::printf("validation done (%d failures); devices: %d; %s\n", g_fail, ndev, hf_version());
  if (ndev > 0) {
    const int layers[2] = {2, 4};
    hf_model_t models[2] = {nullptr, nullptr};
    unsigned seed = 777;
    for (int i = 0; i < 2; ++i) {
      std::vector<float> params((size_t)hf_model_param_count(4, 128, layers[i]));
      for (float &v : params) {
        seed = seed * 1664525u + 1013904223u;
        v = 0.05f * (((seed >> 8) & 0xFFFF) / 65536.0f - 0.5f);
      }
      EXPECT(hf_model_create(params.data(), 4, 128, layers[i], HF_WDTYPE_F32, &models[i]) == HF_OK);
    }
    hf_model_set_t set = nullptr;
    EXPECT(hf_model_set_create(models, 2, &set) == HF_OK && hf_model_set_size(set) == 2);
    if (set) {
      rollouts(set, models, 2, 5, 64, 3);  // fused: one launch, ragged last workgroup per model
      rollouts(set, models, 2, 3, 20, 2);  // not fused: model after model
    }
    hf_model_set_destroy(set);
    hf_model_t odd = nullptr;  // a model the chain kernels do not take
    std::vector<float> p3((size_t)hf_model_param_count(4, 64, 1), 0.01f);
    EXPECT(hf_model_create(p3.data(), 4, 64, 1, HF_WDTYPE_F32, &odd) == HF_OK);
    hf_model_t mixed[2] = {models[0], odd};
    EXPECT(hf_model_set_create(mixed, 2, &set) == HF_EUNSUPPORTED && set == nullptr);
    hf_model_destroy(odd);
    for (hf_model_t m : models) hf_model_destroy(m);
    std::printf("device checks done\n");
  }
  return finish("model_set_sanitize");
}
