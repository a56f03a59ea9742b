// Unrolled training of PureGNN: the residual update of one rollout step with
// the next step's node features and the step's loss term
// (hf_pure_unroll_update), and its adjoint (hf_pure_unroll_adjoint), one launch
// each (scripts/evaluation/evaluate_multi_ic.py:53-64 under a K-step loss;
// include/hybridflux.h has the mathematics).
//
// The two sides of the update live in two layouts: delta is [B*nx][3] (cell,
// channel), the states are [B][3][nx] (channel, cell).  A workgroup owns a tile
// of kPuTile consecutive cells of one IC: the tile's delta block (3 n
// contiguous floats) is read lane after lane into LDS and read back per cell
// (stride 3 words: 3 is odd, so no two lanes of a half wave share a bank), the
// three state rows are read and written lane after lane, and a cell's features
// go out as one 16-byte store.  The adjoint runs the same tile the other way.
// The loss follows unroll.hip: float64 partials, one per workgroup, summed in
// workgroup order by the last wave to arrive.
#include "hf_internal.h"
#include "unroll_common.h"

namespace hf {
namespace {

constexpr int kPuThreads = 256;
constexpr int kPuTile = 1024;  // cells of one IC per workgroup: 12 KiB of LDS per staged block
typedef float pu_f4 __attribute__((ext_vector_type(4)));

inline int64_t tiles_of(int nx) { return ((int64_t)nx + kPuTile - 1) / kPuTile; }

// Workspace: [0, kCounterBytes) the arrival counter, then one float64 loss
// partial per workgroup; the _ex calls with the conservation terms add three
// float64 sums per workgroup behind them (sum u^2, sum E^2, sum n of the tile).
struct LossArgs : StateLossArgs {};  // part [B * tiles]
struct ConsArgs : StateConsArgs {    // part [B * tiles][3]
  int B, nx, tiles;
};

// The step's loss from the per-workgroup partials, by the wave that arrives
// last (unroll.hip's scheme).  Called by a whole wave after its partial store;
// `total` waves call it per launch (arrival_ticket); the partials are summed in
// workgroup order per lane and then across the lanes in a fixed tree, so the
// value does not depend on which wave arrives last.
// EX with the conservation terms: an IC's sums are complete only here, so this
// wave also adds each IC's tiles in tile order (a lane takes ICs lane, lane +
// 64, ...), writes the IC's two coefficients (float64, rounded once) and adds
// the ICs' terms in the same fixed order.
template <bool EX>
__device__ __forceinline__ void loss_arrive(const LossArgs &la, const ConsArgs &ca, unsigned total, int lane) {
  if (arrival_ticket(la.cnt, lane) != total - 1) return;
  acquire_partials();
  const double *part = la.part;
  double a = 0.0;
  for (unsigned i = lane; i < total; i += 64) a += part[i];
  a = wave_sum(a);
  if constexpr (!EX) {
    if (lane == 0) la.loss[0] = (float)(a * la.scale);
  } else {
    double e = 0.0, q = 0.0;
    if (ca.on) {
      const double nx = (double)ca.nx;
      for (int b = lane; b < ca.B; b += 64) {
        const double *t = ca.part + (int64_t)b * ca.tiles * 3;
        double su2 = 0.0, sE2 = 0.0, sn = 0.0;
        for (int j = 0; j < ca.tiles; ++j) su2 += t[3 * j], sE2 += t[3 * j + 1], sn += t[3 * j + 2];
        double pe, pq;
        cons_terms(ca, b, su2, sE2, sn, nx, pe, pq);
        e += pe;
        q += pq;
      }
      e = wave_sum(e);
      q = wave_sum(q);
    }
    if (lane == 0) {
      // (total, state, energy, charge): the state value is the plain call's
      const double ls = a * la.scale, le = e * ca.scale, lq = q * ca.scale;
      la.loss[0] = ca.on ? (float)((ls + le) + lq) : (float)ls;
      la.loss[1] = (float)ls;
      la.loss[2] = (float)le;
      la.loss[3] = (float)lq;
    }
  }
}

// ---------------------------------------------------------------------- forward
// Workgroup blockIdx.x = b * tiles + t owns cells [t kPuTile, t kPuTile + n) of IC b.
template <bool EX>
__global__ __launch_bounds__(kPuThreads) void pure_unroll_update_kernel(const float *__restrict__ delta,
                                                                        const float *__restrict__ in,
                                                                        const float *__restrict__ x, int nx, int tiles,
                                                                        float *__restrict__ out, float *__restrict__ nf,
                                                                        LossArgs la, ConsArgs ca) {
  __shared__ __attribute__((aligned(16))) float Ld[3 * kPuTile];
  __shared__ double red[kPuThreads / 64];
  const int64_t b = blockIdx.x / (unsigned)tiles;
  const int c0 = (int)(blockIdx.x % (unsigned)tiles) * kPuTile;
  const int n = min(kPuTile, nx - c0);
  const float *db = delta + (b * nx + c0) * 3;  // the tile's delta block, (cell, channel) order
  for (int j = threadIdx.x; j < 3 * n; j += kPuThreads) Ld[j] = db[j];
  __syncthreads();
  const int64_t sb = b * 3 * nx + c0;  // row 0 of the tile in the [B][3][nx] tensors
  const float *tg = la.tgt ? la.tgt + sb : nullptr;
  const bool cons = EX && ca.on && tg;
  double acc = 0.0, su2 = 0.0, sE2 = 0.0, sn = 0.0;
  for (int i = threadIdx.x; i < n; i += kPuThreads) {
    const float n_new = __fadd_rn(in[sb + i], Ld[3 * i]);
    const float u_new = __fadd_rn(in[sb + nx + i], Ld[3 * i + 1]);
    const float E_new = __fadd_rn(in[sb + 2 * (int64_t)nx + i], Ld[3 * i + 2]);
    out[sb + i] = n_new;
    out[sb + nx + i] = u_new;
    out[sb + 2 * (int64_t)nx + i] = E_new;
    if (nf) *reinterpret_cast<pu_f4 *>(nf + 4 * (b * nx + c0 + i)) = pu_f4{n_new, u_new, E_new, x[c0 + i]};
    if (tg)
      acc += sq_err(n_new, tg[i], la.w0) + sq_err(u_new, tg[nx + i], la.w1) +
             sq_err(E_new, tg[2 * (int64_t)nx + i], la.w2);
    if (cons) {
      su2 += (double)u_new * (double)u_new;
      sE2 += (double)E_new * (double)E_new;
      sn += (double)n_new;
    }
  }
  if (!tg) return;  // (uniform)
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  if constexpr (EX) {
    __shared__ double redc[3][4];
    if (cons) {  // (uniform)
      su2 = wave_sum(su2);
      sE2 = wave_sum(sE2);
      sn = wave_sum(sn);
      if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        redc[0][wv] = su2, redc[1][wv] = sE2, redc[2][wv] = sn;
      }
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    if (threadIdx.x == 0) la.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    if (cons && threadIdx.x < 3)
      ca.part[(int64_t)blockIdx.x * 3 + threadIdx.x] =
          ((redc[threadIdx.x][0] + redc[threadIdx.x][1]) + redc[threadIdx.x][2]) + redc[threadIdx.x][3];
  } else {
    __syncthreads();
    if (threadIdx.x >= 64) return;
    if (threadIdx.x == 0) la.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
  }
  loss_arrive<EX>(la, ca, gridDim.x, threadIdx.x);
}

// ---------------------------------------------------------------------- adjoint
// grad_delta[cell][ch] = (seed + grad_delta_next[cell][ch]) + grad_nf_next[cell][ch],
// seed = gs_ch (s' - target)[ch][cell]; a NULL term is left out.  EX with coef
// [B][2] = (ce, cq): the seed gains cq_b, ce_b u', ce_b E' on its three
// channels (one float32 product, added to the seed before the other terms).
template <bool EX>
__global__ __launch_bounds__(kPuThreads) void pure_unroll_adjoint_kernel(const float *__restrict__ sn,
                                                                         const float *__restrict__ tgt, float gs0,
                                                                         float gs1, float gs2,
                                                                         const float *__restrict__ gd_next,
                                                                         const float *__restrict__ gnf_next, int nx,
                                                                         int tiles, float *__restrict__ gd,
                                                                         const float *__restrict__ coef) {
  __shared__ __attribute__((aligned(16))) float Ls[3 * kPuTile];  // the seeds, (cell, channel) order
  __shared__ __attribute__((aligned(16))) float Lg[3 * kPuTile];  // columns 0..2 of grad_nf_next
  const int64_t b = blockIdx.x / (unsigned)tiles;
  const int c0 = (int)(blockIdx.x % (unsigned)tiles) * kPuTile;
  const int n = min(kPuTile, nx - c0);
  const int64_t sb = b * 3 * nx + c0;
  float ce = 0.f, cq = 0.f;
  if constexpr (EX) {
    if (coef) ce = coef[2 * b], cq = coef[2 * b + 1];
  }
  for (int i = threadIdx.x; i < n; i += kPuThreads) {
    if constexpr (EX) {
      if (coef) {  // (uniform)
        const float un = sn[sb + nx + i], En = sn[sb + 2 * (int64_t)nx + i];
        Ls[3 * i] = gs0 * (sn[sb + i] - tgt[sb + i]) + cq;
        Ls[3 * i + 1] = gs1 * (un - tgt[sb + nx + i]) + ce * un;
        Ls[3 * i + 2] = gs2 * (En - tgt[sb + 2 * (int64_t)nx + i]) + ce * En;
      }
    }
    if (!EX || !coef) {
      Ls[3 * i] = gs0 * (sn[sb + i] - tgt[sb + i]);
      Ls[3 * i + 1] = gs1 * (sn[sb + nx + i] - tgt[sb + nx + i]);
      Ls[3 * i + 2] = gs2 * (sn[sb + 2 * (int64_t)nx + i] - tgt[sb + 2 * (int64_t)nx + i]);
    }
    if (gnf_next) {
      const pu_f4 g = *reinterpret_cast<const pu_f4 *>(gnf_next + 4 * (b * nx + c0 + i));
      Lg[3 * i] = g.x;
      Lg[3 * i + 1] = g.y;
      Lg[3 * i + 2] = g.z;
    }
  }
  __syncthreads();
  const int64_t db = (b * nx + c0) * 3;
  for (int j = threadIdx.x; j < 3 * n; j += kPuThreads) {
    float v = Ls[j];
    if (gd_next) v = v + gd_next[db + j];
    if (gnf_next) v = v + Lg[j];
    gd[db + j] = v;
  }
}

// one loss partial per tile; cons: three more (sum u^2, sum E^2, sum n)
LossWs carve_pure_unroll_ws(int B, int nx, bool cons, void *base) {
  const size_t n = (size_t)((int64_t)B * tiles_of(nx));
  return carve_loss_ws(n, cons ? 3 * n : 0, base);
}

template <bool EX>
hipError_t update_launch(const float *delta, const float *st, const float *x, int B, int nx, float *st_next,
                         float *nf_next, const float *target, const float *w, float scale, float *loss, void *ws,
                         const ConsTerms *cons, hipStream_t s) {
  const int tiles = (int)tiles_of(nx);
  const unsigned grid = (unsigned)((int64_t)B * tiles);
  LossArgs la{};
  ConsArgs ca{};
  if (target) {
    const hipError_t e = state_loss_setup(la, ca, target, w, scale, loss, carve_pure_unroll_ws(B, nx, cons != nullptr, ws), cons, s);
    if (e) return e;
    if (ca.on) ca.B = B, ca.nx = nx, ca.tiles = tiles;
  }
  hipLaunchKernelGGL(pure_unroll_update_kernel<EX>, dim3(grid), dim3(kPuThreads), 0, s, delta, st, x, nx, tiles, st_next,
                     nf_next, la, ca);
  return hipGetLastError();
}

template <bool EX>
hipError_t adjoint_launch(const float *st_next, const float *target, const float *w, float scale, const float *gd_next,
                          const float *gnf_next, int B, int nx, float *gd, const float *coef, hipStream_t s) {
  const int tiles = (int)tiles_of(nx);
  const unsigned grid = (unsigned)((int64_t)B * tiles);
  float gs[3];
  for (int k = 0; k < 3; ++k) gs[k] = (float)(2.0 * (double)w[k] * (double)scale);
  hipLaunchKernelGGL(pure_unroll_adjoint_kernel<EX>, dim3(grid), dim3(kPuThreads), 0, s, st_next, target, gs[0], gs[1],
                     gs[2], gd_next, gnf_next, nx, tiles, gd, coef);
  return hipGetLastError();
}

}  // namespace

int64_t pure_unroll_ws_bytes(int B, int nx) { return (int64_t)carve_pure_unroll_ws(B, nx, false, nullptr).bytes; }
int64_t pure_unroll_ws_bytes_ex(int B, int nx) { return (int64_t)carve_pure_unroll_ws(B, nx, true, nullptr).bytes; }

// one workgroup per tile: B * tiles of them must fit a grid
bool pure_unroll_shape_ok(int B, int nx) { return B >= 1 && nx >= 1 && (int64_t)B * tiles_of(nx) <= 0x7fffffffLL; }

// ex picks the instantiation; the plain entry points pass cons / coef NULL
hipError_t launch_pure_unroll_update(bool ex, const float *delta, const float *st, const float *x, int B, int nx,
                                     float *st_next, float *nf_next, const float *target, const float *w, float scale,
                                     float *loss, void *ws, const ConsTerms *cons, hipStream_t s) {
  if (!pure_unroll_shape_ok(B, nx)) return hipErrorInvalidValue;
  return (ex ? update_launch<true> : update_launch<false>)(delta, st, x, B, nx, st_next, nf_next, target, w, scale,
                                                            loss, ws, ex ? cons : nullptr, s);
}

hipError_t launch_pure_unroll_adjoint(bool ex, const float *st_next, const float *target, const float *w, float scale,
                                      const float *gd_next, const float *gnf_next, int B, int nx, float *gd,
                                      const float *coef, hipStream_t s) {
  if (!pure_unroll_shape_ok(B, nx)) return hipErrorInvalidValue;
  return (ex ? adjoint_launch<true> : adjoint_launch<false>)(st_next, target, w, scale, gd_next, gnf_next, B, nx, gd,
                                                              coef, s);
}

}  // namespace hf
