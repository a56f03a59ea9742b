// Initial conditions on the device (include/hybridflux.h hf_initial_conditions):
// n and u of src/baseline_solver.py:29-51 for a batch of integer seeds, from the
// same 32-bit words np.random.RandomState(seed) consumes.
//
// The draw protocol (numpy's legacy RandomState over MT19937):
//   seeding   init_genrand: mt[0] = seed, mt[i] = 1812433253 (mt[i-1] ^ mt[i-1] >> 30) + i;
//             the first draw twists the state
//   randint   masked rejection, one word per try
//   rand      (a 2^26 + b) / 2^53 from a = word >> 5, b = next word >> 6
//   randn     polar method, four words per attempt, accepted or not; an accepted
//             attempt yields f x2 first, then f x1
// The small functions below are that protocol, __host__ __device__: the kernel
// and the host-only ic_draws_host (the CPU tests' view of it) share them.
//
// Kernel: one wave (one 64-thread workgroup) per seed, the 624-word state in
// LDS.  Seeding is a serial chain (on the scalar unit: the seed is wave
// uniform).  The twist runs 64 words at a time in index order: word kk needs
// old mt[kk+1] and old mt[kk+397] or new mt[kk-227], which chunks taken in
// order provide.  The mode draws are serial and wave uniform.  The gauss
// attempts sit at a fixed stride of four words behind them, so the 64 lanes
// each take one; a ballot and a prefix count give every accepted attempt its
// pair index, and the accepting lane writes both cells of u (consecutive
// pairs in consecutive accepting lanes: contiguous stores).  The n row is a
// plain loop over cells across lanes.  Every rejection loop is bounded; an IC
// whose draws give up gets NaN (a wrong generator fails a test, it never spins).
//
// The state noise of training (hf_state_noise, hf_gauss_host) runs on the same
// functions: state_noise_kernel draws randn(3 nx) from word 0 through the same
// draw_gauss, gauss_host through the same gauss_fill_host as ic_draws_host.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "hf_internal.h"

// r2 = x1 x1 + x2 x2 and km x + ph must round as numpy's do (the build's
// -ffp-contract=off, restated here for this file)
#pragma STDC FP_CONTRACT OFF

namespace hf {

namespace {

constexpr int kMtN = 624, kMtM = 397;
constexpr int kRandintTries = 64;
constexpr int kNModes = 5, kUModes = 2, kSlots = kNModes + kUModes;
constexpr double kTwoPi = 2.0 * 3.141592653589793;  // 2 * np.pi

__host__ __device__ inline int gauss_attempt_cap(int nx) { return 2 * nx + 256; }
inline int64_t gauss_attempt_cap(int64_t count) { return 2 * count + 256; }  // hf_gauss_host's counts
// state_noise_kernel's mark of a failed sample on its u row (a quiet NaN), read by state_finish_kernel
constexpr uint32_t kNoiseFailMark = 0x7fd0bad5u;

__host__ __device__ inline uint32_t mt_seed_next(uint32_t prev, int i) {
  return 1812433253u * (prev ^ (prev >> 30)) + (uint32_t)i;
}
// new mt[kk] from old mt[kk], old mt[kk+1] and mt[kk+397] (indices mod 624; the last: new once kk >= 227)
__host__ __device__ inline uint32_t mt_twist(uint32_t cur, uint32_t next, uint32_t far) {
  const uint32_t y = (cur & 0x80000000u) | (next & 0x7fffffffu);
  return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
__host__ __device__ inline uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}
__host__ __device__ inline double rand_from(uint32_t w0, uint32_t w1) {
  const int32_t a = (int32_t)(w0 >> 5), b = (int32_t)(w1 >> 6);
  return (a * 67108864.0 + b) / 9007199254740992.0;
}
// one attempt of the polar method from its four words; true: accepted
__host__ __device__ inline bool gauss_try(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, double &x1, double &x2,
                                          double &r2) {
  x1 = 2.0 * rand_from(w0, w1) - 1.0;
  x2 = 2.0 * rand_from(w2, w3) - 1.0;
  r2 = x1 * x1 + x2 * x2;
  return !(r2 >= 1.0 || r2 == 0.0);
}
__host__ __device__ inline double gauss_scale(double r2) { return sqrt(-2.0 * log(r2) / r2); }

// slots 0..4: the n modes (k of them drawn), slots 5, 6: the u modes
struct Modes {
  int k;
  double km[kSlots], amp[kSlots], ph[kSlots];
};

// Src::next() is the next 32-bit word of the stream.
template <class Src>
__host__ __device__ inline bool randint(Src &s, int lo, int hi, int &out) {
  const uint32_t rng = (uint32_t)(hi - 1 - lo);
  uint32_t mask = rng;
  mask |= mask >> 1;
  mask |= mask >> 2;
  mask |= mask >> 4;
  mask |= mask >> 8;
  mask |= mask >> 16;
  for (int t = 0; t < kRandintTries; ++t) {
    const uint32_t v = s.next() & mask;
    if (v <= rng) {
      out = lo + (int)v;
      return true;
    }
  }
  return false;
}
template <class Src>
__host__ __device__ inline double rand01(Src &s) {
  const uint32_t w0 = s.next();
  const uint32_t w1 = s.next();
  return rand_from(w0, w1);
}
// k = randint(3, 6); per mode km = randint(1, 6), amp = a + a rand(), ph = 2 pi rand(); false: a randint gave up
template <class Src>
__host__ __device__ inline bool draw_modes(Src &s, Modes &m) {
  int k = 0;
  if (!randint(s, 3, 6, k)) return false;
  m.k = k;
  for (int slot = 0; slot < kSlots; ++slot) {
    if (slot < kNModes && slot >= k) continue;
    int km = 0;
    if (!randint(s, 1, 6, km)) return false;
    const double a = slot < kNModes ? 0.15 : 0.1;
    m.km[slot] = (double)km;
    m.amp[slot] = a + a * rand01(s);
    m.ph[slot] = kTwoPi * rand01(s);
  }
  return true;
}

__host__ __device__ inline void write_table(double *t, const Modes &m, bool ok, int64_t words) {
  t[0] = ok ? (double)m.k : -1.0;
  for (int s = 0; s < kSlots; ++s) {
    t[1 + 3 * s] = m.km[s];
    t[2 + 3 * s] = m.amp[s];
    t[3 + 3 * s] = m.ph[s];
  }
  t[HF_IC_TABLE_LEN - 1] = (double)words;
}

// ---- host ----------------------------------------------------------------------
struct HostSrc {
  uint32_t mt[kMtN];
  int pos = kMtN;
  int64_t words = 0;
  explicit HostSrc(uint32_t seed) {
    mt[0] = seed;
    for (int i = 1; i < kMtN; ++i) mt[i] = mt_seed_next(mt[i - 1], i);
  }
  uint32_t next() {
    if (pos == kMtN) {
      for (int kk = 0; kk < kMtN; ++kk)
        mt[kk] = mt_twist(mt[kk], mt[kk + 1 == kMtN ? 0 : kk + 1], mt[kk + kMtM < kMtN ? kk + kMtM : kk + kMtM - kMtN]);
      pos = 0;
    }
    ++words;
    return mt_temper(mt[pos++]);
  }
};

// randn(count) from the stream's next word on; at most cap attempts (false: they ran out)
inline bool gauss_fill_host(HostSrc &src, int64_t count, int64_t cap, double *gauss) {
  const int64_t npairs = (count + 1) / 2;
  int64_t p = 0;
  for (int64_t j = 0; p < npairs; ++j) {
    if (j >= cap) return false;
    const uint32_t w0 = src.next(), w1 = src.next(), w2 = src.next(), w3 = src.next();
    double x1, x2, r2;
    if (!gauss_try(w0, w1, w2, w3, x1, x2, r2)) continue;
    const double f = gauss_scale(r2);
    gauss[2 * p] = f * x2;
    if (2 * p + 1 < count) gauss[2 * p + 1] = f * x1;
    ++p;
  }
  return true;
}

// ---- device --------------------------------------------------------------------
// The stream as one wave sees it: mt[] holds block `base / 624` of the word
// stream, pos is the next unread word of it, carry[] the last three words of
// the block before (a gauss attempt may straddle the boundary).
struct DevSrc {
  uint32_t *mt, *carry;
  int lane, pos, base;

  __device__ void twist() {
    for (int c = 0; c < kMtN; c += 64) {
      const int kk = c + lane;
      const bool on = kk < kMtN;
      uint32_t v = 0;
      if (on) {
        const int nx1 = kk + 1 == kMtN ? 0 : kk + 1;
        const int far = kk + kMtM < kMtN ? kk + kMtM : kk + kMtM - kMtN;
        v = mt_twist(mt[kk], mt[nx1], mt[far]);
      }
      __syncthreads();
      if (on) mt[kk] = v;
      __syncthreads();
    }
  }
  __device__ void seed(uint32_t s) {
    uint32_t v = s;
    if (lane == 0) mt[0] = v;
    for (int i = 1; i < kMtN; ++i) {
      v = mt_seed_next(v, i);
      if (lane == 0) mt[i] = v;
    }
    __syncthreads();
    twist();
    pos = 0;
    base = 0;
  }
  __device__ void advance() {
    __syncthreads();
    if (lane < 3) carry[lane] = mt_temper(mt[kMtN - 3 + lane]);
    twist();
    base += kMtN;
    pos = 0;
  }
  // serial, wave-uniform draws
  __device__ uint32_t next() {
    if (pos == kMtN) advance();
    const uint32_t v = mt_temper(mt[pos]);
    ++pos;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
  }
  // word g of the stream, base - 3 <= g < base + 624
  __device__ uint32_t at(int g) const {
    const int r = g - base;
    return r >= 0 ? mt_temper(mt[r]) : carry[r + 3];
  }
};

// randn(count) from the next unread word on, by the whole wave: the attempts
// sit at a fixed stride of four words, so the 64 lanes each take one; a ballot
// and a prefix count give every accepted attempt its pair index p, and the
// accepting lane hands put(2 p, f x2) and put(2 p + 1, f x1) (consecutive pairs
// in consecutive accepting lanes).  At most cap attempts; false: they ran out.
// words: the stream's first word after the last accepted attempt.
template <class Put>
__device__ inline bool draw_gauss(DevSrc &src, int count, int cap, int &words, Put put) {
  const int npairs = (count + 1) / 2;
  const int lane = src.lane;
  const int w0 = src.base + src.pos;  // attempt j reads words w0 + 4 j .. + 3
  int acc = 0, jn = 0, jlast = -1;
  bool ok = true;
  for (;;) {
    int avail = (src.base + kMtN - w0) / 4;  // attempts that end inside the blocks generated so far
    avail = avail < cap ? avail : cap;
    while (jn < avail && acc < npairs) {
      const int j = jn + lane;
      bool hit = false;
      double x1 = 0.0, x2 = 0.0, r2 = 1.0;
      if (j < avail) {
        const int g = w0 + 4 * j;
        hit = gauss_try(src.at(g), src.at(g + 1), src.at(g + 2), src.at(g + 3), x1, x2, r2);
      }
      const unsigned long long hits = __ballot(hit);
      const int p = acc + __popcll(hits & ((1ull << lane) - 1ull));
      if (hit && p < npairs) {
        const double f = gauss_scale(r2);
        put(2 * p, f * x2);
        if (2 * p + 1 < count) put(2 * p + 1, f * x1);
      }
      const unsigned long long last = __ballot(hit && p == npairs - 1);
      if (last) jlast = jn + __ffsll((long long)last) - 1;
      acc += __popcll(hits);
      jn = jn + 64 < avail ? jn + 64 : avail;
    }
    if (acc >= npairs) break;
    if (jn >= cap) {
      ok = false;
      break;
    }
    src.advance();
  }
  words = w0 + 4 * (jlast + 1);
  return ok;
}

__global__ __launch_bounds__(64) void initial_conditions_kernel(const int64_t *__restrict__ seeds, int nx,
                                                                const double *__restrict__ x,
                                                                float *__restrict__ state,
                                                                double *__restrict__ table) {
  __shared__ uint32_t mt[kMtN];
  __shared__ uint32_t carry[4];
  __shared__ Modes modes;
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  float *n = state + b * 3 * nx, *u = n + nx;

  if (lane < kSlots) modes.km[lane] = modes.amp[lane] = modes.ph[lane] = 0.0;
  if (lane == 0) modes.k = 0;
  __syncthreads();

  const int64_t seed = seeds[b];
  bool ok = seed >= 0 && seed <= 0xffffffffLL;
  int words = 0;
  if (ok) {
    DevSrc src{mt, carry, lane, 0, 0};
    src.seed((uint32_t)seed);
    ok = draw_modes(src, modes);
    if (ok) {
      __syncthreads();
      const int k = __builtin_amdgcn_readfirstlane(modes.k);
      for (int i = lane; i < nx; i += 64) {
        const double xi = x[i];
        float v = 1.0f;
        for (int m = 0; m < k; ++m) v += (float)modes.amp[m] * (float)sin(modes.km[m] * xi + modes.ph[m]);
        n[i] = v;
      }

      const double km0 = modes.km[kNModes], ph0 = modes.ph[kNModes];
      const double km1 = modes.km[kNModes + 1], ph1 = modes.ph[kNModes + 1];
      const float a0 = (float)modes.amp[kNModes], a1 = (float)modes.amp[kNModes + 1];
      auto u_of = [&](int i, double gauss) {
        const double xi = x[i];
        float v = 0.0f;
        v += a0 * (float)cos(km0 * xi + ph0);
        v += a1 * (float)cos(km1 * xi + ph1);
        v += 0.05f * (float)gauss;
        return v;
      };
      ok = draw_gauss(src, nx, gauss_attempt_cap(nx), words, [&](int i, double gauss) { u[i] = u_of(i, gauss); });
    }
  }
  if (!ok) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = lane; i < nx; i += 64) n[i] = u[i] = nan;
  }
  if (table && lane == 0) write_table(table + b * HF_IC_TABLE_LEN, modes, ok, words);
}

// Seeded Gaussian state noise (include/hybridflux.h hf_state_noise): one wave
// per sample draws g = randn(3 nx) from word 0 of its seed's stream and adds
// f32(s_ch) * f32(g) to rows n, u, E of in [B][3][nx] as the values are
// accepted (out may be in: a cell is read and written by the same lane).  hold
// (zero mean on a perturbed n row): g_n waits in gn[nx] (dynamic LDS) for its
// mean -- a lane's cells in ascending order, the lanes in the xor tree -- and
// the n row is a second pass.  Rows with s_ch == 0 are copied as bits; with
// skip_E row E of out is not touched (the caller's Poisson launch writes it).
// A bad seed or draws that give up: NaN in noise and, without skip_E, in all
// three rows.  With skip_E the sample's n row must stay finite for the Poisson
// launch, which at the FFT sizes transforms two samples as one complex row: n
// is filled with 1 (rho = 0), u with kNoiseFailMark, and state_finish_kernel
// turns the sample NaN after the solve.
__global__ __launch_bounds__(64) void state_noise_kernel(const int64_t *__restrict__ seeds, int nx, float s_n, float s_u,
                                                         float s_E, bool hold, bool skip_E, const float *in, float *out,
                                                         float *noise) {
  __shared__ uint32_t mt[kMtN];
  __shared__ uint32_t carry[4];
  extern __shared__ double gn[];
  const int lane = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * 3 * nx;
  const float *si = in + row;
  float *so = out + row, *nz = noise ? noise + row : nullptr;
  auto sigma = [&](int ch) { return ch == 0 ? s_n : ch == 1 ? s_u : s_E; };
  auto added = [&](int ch) { return sigma(ch) != 0.0f && !(ch == 2 && skip_E); };
  auto add = [&](int ch, int i, double d) {
    if (!added(ch)) return;
    const int64_t o = (int64_t)ch * nx + i;
    const float a = sigma(ch) * (float)d;
    so[o] = si[o] + a;
    if (nz) nz[o] = a;
  };

  const int64_t seed = seeds[blockIdx.x];
  bool ok = seed >= 0 && seed <= 0xffffffffLL;
  if (ok) {
    DevSrc src{mt, carry, lane, 0, 0};
    src.seed((uint32_t)seed);
    int words = 0;
    ok = draw_gauss(src, 3 * nx, gauss_attempt_cap(3 * nx), words, [&](int j, double g) {
      const int ch = j >= 2 * nx ? 2 : j >= nx ? 1 : 0;
      if (hold && ch == 0)
        gn[j] = g;
      else
        add(ch, j - ch * nx, g);
    });
    if (ok && hold) {
      __syncthreads();
      double acc = 0.0;
      for (int i = lane; i < nx; i += 64) acc += gn[i];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
      const double m = acc / (double)nx;
      for (int i = lane; i < nx; i += 64) add(0, i, gn[i] - m);
    }
  }
  const uint32_t *bi = reinterpret_cast<const uint32_t *>(si);
  uint32_t *bo = reinterpret_cast<uint32_t *>(so);
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (int ch = 0; ch < 3; ++ch) {
    if (ok && added(ch)) continue;
    const bool recomputed = ch == 2 && skip_E;
    for (int i = lane; i < nx; i += 64) {
      const int64_t o = (int64_t)ch * nx + i;
      if (!ok) {
        if (!skip_E)
          so[o] = nan;
        else if (ch == 0)
          so[o] = 1.0f;
        else if (ch == 1)
          bo[o] = kNoiseFailMark;
        if (nz) nz[o] = nan;
        continue;
      }
      if (!recomputed && so != si) bo[o] = bi[o];
      if (nz) nz[o] = 0.0f;
    }
  }
}

// The pass behind the Poisson launch, one wave per sample.  seal: a sample
// whose u row holds kNoiseFailMark in every cell (state_noise_kernel's failed
// sample) gets NaN in all three rows.  nf (or NULL): [B nx][4] = [n, u, E, x]
// of the state as it then stands, exact copies.
__global__ __launch_bounds__(64) void state_finish_kernel(float *__restrict__ st, const float *__restrict__ x, int nx,
                                                          bool seal, float *__restrict__ nf) {
  const int lane = threadIdx.x;
  float *s = st + (int64_t)blockIdx.x * 3 * nx;
  bool failed = false;
  if (seal) {
    const uint32_t *u = reinterpret_cast<const uint32_t *>(s + nx);
    bool marked = true;
    for (int i = lane; i < nx; i += 64) marked = marked && u[i] == kNoiseFailMark;
    failed = __all(marked);
  }
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (int i = lane; i < nx; i += 64) {
    float v[3];
    for (int ch = 0; ch < 3; ++ch) {
      v[ch] = failed ? nan : s[(int64_t)ch * nx + i];
      if (failed) s[(int64_t)ch * nx + i] = nan;
    }
    if (nf) {
      float *f = nf + 4 * ((int64_t)blockIdx.x * nx + i);
      f[0] = v[0];
      f[1] = v[1];
      f[2] = v[2];
      f[3] = x[i];
    }
  }
}

}  // namespace

hipError_t launch_initial_conditions(const int64_t *seeds, int B, int nx, const double *x, float *state, double *table,
                                     hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (nx < 1 || nx > kIcMaxNx) return hipErrorInvalidValue;
  hipLaunchKernelGGL(initial_conditions_kernel, dim3((unsigned)B), dim3(64), 0, s, seeds, nx, x, state, table);
  return hipGetLastError();
}

bool ic_draws_host(int64_t seed, int nx, double *table, double *gauss) {
  if (seed < 0 || seed > 0xffffffffLL || nx < 1 || nx > kIcMaxNx) return false;
  HostSrc src((uint32_t)seed);
  Modes m{};
  const bool ok = draw_modes(src, m) && gauss_fill_host(src, nx, gauss_attempt_cap(nx), gauss);
  if (!ok)
    for (int i = 0; i < nx; ++i) gauss[i] = std::numeric_limits<double>::quiet_NaN();
  write_table(table, m, ok, src.words);
  return true;
}

hipError_t launch_state_noise(const int64_t *seeds, int B, int nx, const float *sig, bool zero_mean, bool skip_E,
                              const float *in, float *out, float *noise, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (nx < 1 || nx > kIcMaxNx || (zero_mean && nx > kNoiseZeroMeanMaxNx)) return hipErrorInvalidValue;
  // g_n waits in LDS for its mean only when the n row is perturbed at all
  const bool hold = zero_mean && sig[0] != 0.0f;
  hipLaunchKernelGGL(state_noise_kernel, dim3((unsigned)B), dim3(64), hold ? sizeof(double) * (size_t)nx : 0, s, seeds,
                     nx, sig[0], sig[1], sig[2], hold, skip_E, in, out, noise);
  return hipGetLastError();
}

hipError_t launch_state_finish(float *state, const float *x, int B, int nx, bool seal, float *nf, hipStream_t s) {
  if (B <= 0 || (!seal && !nf)) return hipSuccess;
  if (nx < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(state_finish_kernel, dim3((unsigned)B), dim3(64), 0, s, state, x, nx, seal, nf);
  return hipGetLastError();
}

bool gauss_host(int64_t seed, int64_t count, double *gauss) {
  if (seed < 0 || seed > 0xffffffffLL || count < 0 || count > 3LL * kIcMaxNx) return false;
  HostSrc src((uint32_t)seed);
  if (!gauss_fill_host(src, count, gauss_attempt_cap(count), gauss))
    for (int64_t i = 0; i < count; ++i) gauss[i] = std::numeric_limits<double>::quiet_NaN();
  return true;
}

}  // namespace hf
