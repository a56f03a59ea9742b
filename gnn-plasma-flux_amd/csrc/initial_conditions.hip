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
      const int npairs = (nx + 1) / 2, cap = gauss_attempt_cap(nx);
      const int w0 = src.base + src.pos;  // attempt j reads words w0 + 4 j .. + 3
      int acc = 0, jn = 0, jlast = -1;
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
            u[2 * p] = u_of(2 * p, f * x2);
            if (2 * p + 1 < nx) u[2 * p + 1] = u_of(2 * p + 1, f * x1);
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
    }
  }
  if (!ok) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = lane; i < nx; i += 64) n[i] = u[i] = nan;
  }
  if (table && lane == 0) write_table(table + b * HF_IC_TABLE_LEN, modes, ok, words);
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
  bool ok = draw_modes(src, m);
  const int npairs = (nx + 1) / 2, cap = gauss_attempt_cap(nx);
  int p = 0;
  for (int j = 0; ok && p < npairs; ++j) {
    if (j >= cap) {
      ok = false;
      break;
    }
    const uint32_t w0 = src.next(), w1 = src.next(), w2 = src.next(), w3 = src.next();
    double x1, x2, r2;
    if (!gauss_try(w0, w1, w2, w3, x1, x2, r2)) continue;
    const double f = gauss_scale(r2);
    gauss[2 * p] = f * x2;
    if (2 * p + 1 < nx) gauss[2 * p + 1] = f * x1;
    ++p;
  }
  if (!ok)
    for (int i = 0; i < nx; ++i) gauss[i] = std::numeric_limits<double>::quiet_NaN();
  write_table(table, m, ok, src.words);
  return true;
}

}  // namespace hf
