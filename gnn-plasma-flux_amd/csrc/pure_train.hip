// PureGNN training (scripts/training/train_pure_gnn.py:59-76 under
// batch_loss.backward(), :100-151): the forward that keeps an activation tape,
// the backward, and the fused state-MSE loss of :134-141 with its gradient.
//
// Forward: the arithmetic of the inference forward (baselines.hip
// pure_forward), launch for launch, so delta is bit-identical to it on either
// path; every message tanh(P[src] + Q[dst] + b) is also written to the tape, so
// the backward recomputes no tanh.
//
// Tape (PureTape; every piece 256-byte aligned, in this order):
//   buckets   carve_edge_buckets(N, E): the CSR of the edges by dst (general
//             graphs only; chains find their neighbours arithmetically)
//   h[0..L]   [N][H] each: h_0 = tanh(W_in nf + b_in), h_{l+1} = h_l + sum of messages
//   z         [N][H]: tanh(W_o1 h_L + b_o1)
//   m[0..L)   the messages of layer l, E * H floats each.  chain_nx > 0:
//             [N][2][H], row 2i the message into cell i from i-1 (m-), row
//             2i+1 the one from i+1 (m+), periodic per chain.  Otherwise [E][H],
//             row e the message of edge e.
//   q         [N][H] scratch of the generic forward (L > 0)
//
// Backward, given g_delta [N][3] (the math of hf_pure_gnn_backward's comment):
//   head     a = (g_delta W_o2) * (1 - z^2); gW_o2, gW_o1 and their biases;
//            g_L = a W_o1
//   layer l  gQ[d] = sum_{e: dst = d} g'[d] (1 - m_e^2), gP[s] = sum_{e: src = s}
//            g'[dst_e] (1 - m_e^2), both over ascending e (chains: two terms
//            each; general graphs: the CSR by dst of the tape and a CSR by src
//            built here), no atomics; gW_l = [gP^T h_l | gQ^T h_l], gb_l = column
//            sums of gQ; g_l = g' + [gP | gQ] [W_a ; W_b]
//   input    a_0 = g_0 * (1 - h_0^2); gW_in, gb_in; g_nf = a_0 W_in (on request)
// Two paths, chosen as the inference forward chooses (pure_chain_ok: tagged
// chains with nx | 128 and H % 64 == 0):
//   chain    tgemm.h GEMMs: the data gradients with the residual and tanh'
//            in the epilogue (EpiGrad), the L layers' weight gradients as ONE
//            split-K launch (tgemm_batch over [gP | gQ]^T h_l with COLSUM for
//            the bias) and one fixed-order reduction of all their partials
//   generic  gemm_linear / gemm_wgrad of graph.hip (any graph, width, nx)
// The K = 3 and K = in_dim GEMMs (output_mlp.2, input_mlp.0) are generic on both.
// Every sum has a fixed order: two backward passes give the same bits.
#include <algorithm>

#include "hf_device.h"
#include "hf_internal.h"
#include "tgemm.h"

namespace hf {
namespace {

using namespace tg;

struct PureTape {
  EdgeBuckets buckets;
  float *h[kMaxChainLayers + 1];
  float *z;
  float *m[kMaxChainLayers];
  float *q;  // [N][H] scratch of the generic forward (Q of the layer in flight; its P is parked in z)
  size_t bytes;
};

PureTape carve_pure_tape(int H, int L, int64_t N, int64_t E, void *base) {
  Carve c(base);
  PureTape t{};
  t.buckets = carve_edge_buckets(c, N, E);
  for (int l = 0; l <= L; ++l) t.h[l] = c.take<float>(N * H);
  t.z = c.take<float>(N * H);
  for (int l = 0; l < L; ++l) t.m[l] = c.take<float>(E * H);
  t.q = c.take<float>(L > 0 ? N * H : 0);
  t.bytes = c.off;
  return t;
}

__device__ __forceinline__ float tanh_bwd(float g, float y) { return __fmul_rn(g, __fsub_rn(1.f, __fmul_rn(y, y))); }

// message_sum_kernel of baselines.hip (the same sums in the same order), also
// writing each message to the tape.
__global__ void message_tape_kernel(const float *__restrict__ h, const float *__restrict__ P,
                                    const float *__restrict__ Q, const float *__restrict__ b,
                                    const int64_t *__restrict__ src, const int *__restrict__ off,
                                    const int *__restrict__ perm, int chain_nx, int64_t N, int H,
                                    float *__restrict__ h_out, float *__restrict__ m) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * H) return;
  const int64_t d = t / H;
  const int f = (int)(t - d * H);
  const float q = Q[t], bf = b[f];
  float acc = 0.f;
  if (chain_nx > 0) {
    const float m0 = tanhf(__fadd_rn(__fadd_rn(P[chain_prev(d, chain_nx) * H + f], q), bf));
    const float m1 = tanhf(__fadd_rn(__fadd_rn(P[chain_next(d, chain_nx) * H + f], q), bf));
    m[2 * d * H + f] = m0;
    m[(2 * d + 1) * H + f] = m1;
    acc = __fadd_rn(__fadd_rn(acc, m0), m1);
  } else {
    for (int p = off[d]; p < off[d + 1]; ++p) {
      const int64_t e = perm[p];
      const float v = tanhf(__fadd_rn(__fadd_rn(P[src[e] * H + f], q), bf));
      m[e * H + f] = v;
      acc = __fadd_rn(acc, v);
    }
  }
  h_out[t] = __fadd_rn(h[t], acc);
}

// EpiMsg of tgemm.h (the inference chain layer's block epilogue, the same
// arithmetic) that also writes the two messages of every cell to the tape.
struct EpiMsgTape {
  const float *h;
  float *out;
  const float *b;
  int H, nx;
  float *m;  // [N][2][H]
  static constexpr bool kPre = false, kBlock = true;
  __device__ float bias_of(int64_t) const { return 0.f; }
  __device__ float pre(int64_t, int64_t) const { return 0.f; }
  __device__ void operator()(int64_t, int64_t, float, float, float) const {}
  static constexpr int kS = EpiMsg::kS;
  __device__ void block(const f16 (&acc)[2][2], float *sP, float *sQ, int64_t i0, int64_t j0, int64_t I, int wi, int wj,
                        int lane, int t) const {
    float *dst = wj == 0 ? sP : sQ;
    const int hl = lane >> 5;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int v = 0; v < 16; ++v)
          dst[(64 * wi + 32 * a + 8 * (v >> 2) + 4 * hl + (v & 3)) * kS + 32 * bb + (lane & 31)] = acc[a][bb][v];
    __syncthreads();
    const int f = t & 63;
    const int64_t fg = (j0 >> 7) * 64 + f;
    const float bf = b[fg];
#pragma unroll 4
    for (int k = 0; k < 32; ++k) {
      const int r = (t >> 6) + 4 * k;
      const int64_t i = i0 + r;
      if (i >= I) break;
      const int ci = (int)((unsigned)i % (unsigned)nx);
      const int rp = r + (ci == 0 ? nx - 1 : -1), rn = r + (ci == nx - 1 ? 1 - nx : 1);
      const float q = sQ[r * kS + f];
      const float m0 = tanhf(__fadd_rn(__fadd_rn(sP[rp * kS + f], q), bf));
      const float m1 = tanhf(__fadd_rn(__fadd_rn(sP[rn * kS + f], q), bf));
      m[2 * i * H + fg] = m0;
      m[(2 * i + 1) * H + fg] = m1;
      out[i * H + fg] = __fadd_rn(h[i * H + fg], __fadd_rn(m0, m1));
    }
  }
};

// [W_a ; W_b] of a message layer (nn.Linear [H][2H]) with its rows along the
// reduction: row r < H is W[r][0..H), row H + r is W[r][H..2H) (any H % 4 == 0).
struct VWab {
  const float *W;
  int H;
  struct Row {
    int off;
  };
  __device__ Row row(int64_t r) const {
    r = r < 2 * H ? r : 2 * H - 1;
    return Row{r < H ? (int)r * 2 * H : ((int)r - H) * 2 * H + H};
  }
  __device__ f4 load4(const Row &w, int c) const {
    c = c < H ? c : H - 4;
    return *reinterpret_cast<const f4 *>(W + (unsigned)(w.off + c));
  }
  __device__ void load2(const Row &w, int c, f4 &a, f4 &) const { a = load4(w, c); }
  __device__ f4 combine(int, const f4 &a, const f4 &) const { return a; }
  bool fits32() const { return 2LL * H * H < (int64_t(1) << 31); }
};

// Data-gradient epilogue: out = (resid + v) * (1 - y^2), resid and y optional
// (neither may alias out).
struct EpiGrad {
  float *out;
  int64_t ld;
  const float *resid, *y;
  __device__ float bias_of(int64_t) const { return 0.f; }
  static constexpr bool kPre = false, kBlock = false;
  __device__ float pre(int64_t, int64_t) const { return 0.f; }
  __device__ void operator()(int64_t i, int64_t j, float v, float, float) const {
    if (resid) v = __fadd_rn(resid[i * ld + j], v);
    if (y) v = tanh_bwd(v, y[i * ld + j]);
    out[i * ld + j] = v;
  }
};

// a[n][f] = (sum_c g[n][c] W_o2[c][f]) * (1 - z[n][f]^2)
__global__ void head_delta_kernel(const float *__restrict__ g, const float *__restrict__ W2,
                                  const float *__restrict__ z, int64_t N, int H, float *__restrict__ a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * H) return;
  const int64_t n = t / H;
  const int f = (int)(t - n * H);
  float v = __fmul_rn(g[3 * n], W2[f]);
  v = __fadd_rn(v, __fmul_rn(g[3 * n + 1], W2[H + f]));
  v = __fadd_rn(v, __fmul_rn(g[3 * n + 2], W2[2 * H + f]));
  a[t] = tanh_bwd(v, z[t]);
}

// out = g * (1 - y^2)
__global__ void tanh_grad_kernel(const float *__restrict__ g, const float *__restrict__ y, int64_t n,
                                 float *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = tanh_bwd(g[t], y[t]);
}

// Message backward on chains (tape rows 2i = m-[i], 2i+1 = m+[i]): with
// a-[i] = g[i] (1 - m-[i]^2), a+[i] likewise,
//   gQ[i] = a-[i] + a+[i]            (edges i-1 and nx+i into cell i)
//   gP[s] = a-[s+1] + a+[s-1]        (edges s and nx+s-1 out of cell s)
// gP / gQ rows ld floats apart.
__global__ void msg_backward_chain_kernel(const float *__restrict__ g, const float *__restrict__ m, int nx, int64_t N,
                                          int H, float *__restrict__ gP, float *__restrict__ gQ, int64_t ld) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * H) return;
  const int64_t i = t / H;
  const int f = (int)(t - i * H);
  const int64_t ip = chain_prev(i, nx), in = chain_next(i, nx);
  const float gi = g[t];
  gQ[i * ld + f] = __fadd_rn(tanh_bwd(gi, m[2 * i * H + f]), tanh_bwd(gi, m[(2 * i + 1) * H + f]));
  gP[i * ld + f] = __fadd_rn(tanh_bwd(g[in * H + f], m[2 * in * H + f]), tanh_bwd(g[ip * H + f], m[(2 * ip + 1) * H + f]));
}

// Message backward on a general graph (tape row e = m_e): the edges into node
// j from the CSR by dst, the edges out of it from the CSR by src, each bucket
// in ascending edge order.
__global__ void msg_backward_csr_kernel(const float *__restrict__ g, const float *__restrict__ m,
                                        const int64_t *__restrict__ dst, const int *__restrict__ off_d,
                                        const int *__restrict__ perm_d, const int *__restrict__ off_s,
                                        const int *__restrict__ perm_s, int64_t N, int H, float *__restrict__ gP,
                                        float *__restrict__ gQ, int64_t ld) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * H) return;
  const int64_t j = t / H;
  const int f = (int)(t - j * H);
  const float gj = g[t];
  float q = 0.f, p = 0.f;
  for (int k = off_d[j]; k < off_d[j + 1]; ++k) q = __fadd_rn(q, tanh_bwd(gj, m[(int64_t)perm_d[k] * H + f]));
  for (int k = off_s[j]; k < off_s[j + 1]; ++k) {
    const int64_t e = perm_s[k];
    p = __fadd_rn(p, tanh_bwd(g[dst[e] * H + f], m[e * H + f]));
  }
  gQ[j * ld + f] = q;
  gP[j * ld + f] = p;
}

// The fixed-order reduction of split-K partials (EpiPart's [S][I][J] and
// COLSUM's [S][I]) of up to kMaxChainLayers problems in one launch (grid y =
// problem).  split = 0: gw[i][j] (rows J apart), gb[i].  split = 1 (I = 2H: the
// rows of [gP | gQ]^T h): row i < H is gw[i][0..J), row H + i is gw[i][J..2J)
// of nn.Linear's [H][2J], and gb the column sums of the gQ half.
struct PrBatch {
  const float *part[kMaxChainLayers], *bpart[kMaxChainLayers];
  float *gw[kMaxChainLayers], *gb[kMaxChainLayers];
};
__global__ __launch_bounds__(256) void pure_part_reduce_kernel(PrBatch b, int S, int I, int J, int split) {
  const int pb = blockIdx.y;
  const int64_t n = (int64_t)I * J, t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n + I) return;
  const bool is_w = t < n;
  const float *src = is_w ? b.part[pb] + t : b.bpart[pb] + (t - n);
  const int64_t st = is_w ? n : I;
  float v = 0.f;
  for (int s = 0; s < S; ++s) v = __fadd_rn(v, src[(int64_t)s * st]);
  const int H = I / 2;
  if (is_w) {
    const int i = (int)(t / J), j = (int)(t - (int64_t)i * J);
    if (split) b.gw[pb][(int64_t)(i < H ? i : i - H) * 2 * J + (i < H ? 0 : J) + j] = v;
    else b.gw[pb][t] = v;
  } else {
    const int i = (int)(t - n);
    if (!split) b.gb[pb][i] = v;
    else if (i >= H) b.gb[pb][i - H] = v;
  }
}

// weight-gradient splits of the chain path: at least 256 rows each, at most 64
inline int pure_wg_splits(int64_t N) { return (int)std::min<int64_t>(64, std::max<int64_t>(1, N / 256)); }

// chain path: the inference forward's (pure_chain_ok) with 32-bit offsets into [N][2H]
bool pure_train_chain(int H, int chain_nx, int64_t N) {
  return pure_chain_ok(H, chain_nx, N) && (N + 1) * 2 * H < (int64_t(1) << 31);
}

struct PureBws {
  EdgeBuckets buckets;           // CSR by src
  float *a, *g[2];               // [N][H]
  float *gpq[kMaxChainLayers];   // [N][2H] per layer ([gP | gQ]; generic path: gP then gQ, [N][H] each, in gpq[0])
  float *gpart;                  // generic split-K partials
  float *hpart, *hbpart;         // chain: head partials [S][H][H], [S][H]
  float *lpart[kMaxChainLayers], *lbpart[kMaxChainLayers];  // chain: layer partials [S][2H][H], [S][2H]
  size_t bytes;
};

PureBws carve_pure_bws(int in_dim, int H, int L, int64_t N, int64_t E, void *base) {
  Carve c(base);
  PureBws w{};
  w.buckets = carve_edge_buckets(c, N, E);
  w.a = c.take<float>(N * H);
  w.g[0] = c.take<float>(N * H);
  w.g[1] = c.take<float>(N * H);
  for (int l = 0; l < std::max(L, 1); ++l) w.gpq[l] = c.take<float>(N * 2 * H);
  const int64_t gp = std::max(gemm_wgrad_part_floats(N, 3, H),
                              std::max(gemm_wgrad_part_floats(N, H, H), gemm_wgrad_part_floats(N, H, in_dim)));
  w.gpart = c.take<float>(gp);
  const int64_t S = tgemm_splits(N, pure_wg_splits(N));
  w.hpart = c.take<float>(S * H * H);
  w.hbpart = c.take<float>(S * H);
  for (int l = 0; l < L; ++l) {
    w.lpart[l] = c.take<float>(S * 2 * H * H);
    w.lbpart[l] = c.take<float>(S * 2 * H);
  }
  w.bytes = c.off;
  return w;
}

// loss partials: block b sums (pred - target)^2 of elements b*256 + t + k * 256 * gridDim.x
// (k ascending) per thread, then its 256 thread sums as a tree; d_delta alongside.
constexpr int kMseBlocks = 1024;
__device__ __forceinline__ float block_sum256(float v, float *sm) {
  const int t = threadIdx.x;
  sm[t] = v;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) sm[t] = __fadd_rn(sm[t], sm[t + w]);
    __syncthreads();
  }
  return sm[0];
}
__global__ __launch_bounds__(256) void state_mse_kernel(const float *__restrict__ delta, const float *__restrict__ st,
                                                        const float *__restrict__ sn, int64_t n, int nx, float scale,
                                                        float *__restrict__ gd, float *__restrict__ part) {
  __shared__ float sm[256];
  float acc = 0.f;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int64_t node = t / 3;
    const int c = (int)(t - node * 3);
    const int64_t b = node / nx;
    const int i = (int)(node - b * nx);
    const int64_t k = (b * 3 + c) * nx + i;
    const float d = __fsub_rn(__fadd_rn(st[k], delta[t]), sn[k]);
    gd[t] = __fmul_rn(d, scale);
    acc = __fadd_rn(acc, __fmul_rn(d, d));
  }
  const float r = block_sum256(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}
__global__ __launch_bounds__(256) void state_mse_final_kernel(const float *__restrict__ part, int nb, float inv_n,
                                                              float *__restrict__ loss) {
  __shared__ float sm[256];
  float acc = 0.f;
  for (int k = threadIdx.x; k < nb; k += 256) acc = __fadd_rn(acc, part[k]);
  const float r = block_sum256(acc, sm);
  if (threadIdx.x == 0) loss[0] = __fmul_rn(r, inv_n);
}

// state_mse_kernel's blocks over n elements; its workspace: one partial each
inline int mse_blocks(int64_t n) { return (int)std::min<int64_t>(kMseBlocks, (n + 255) / 256); }

}  // namespace

int64_t pure_tape_bytes(int H, int L, int64_t N, int64_t E) {
  return (int64_t)carve_pure_tape(H, L, N, E, nullptr).bytes;
}

int64_t pure_backward_ws_bytes(int in_dim, int H, int L, int64_t N, int64_t E) {
  return (int64_t)carve_pure_bws(in_dim, H, L, N, E, nullptr).bytes;
}

hipError_t launch_pure_forward_train(const float *params, int in_dim, int H, int L, const float *nf, int64_t N,
                                     const int64_t *ei, int64_t E, int chain_nx, float *delta, void *tape,
                                     hipStream_t s) {
  const PureW w = pure_view(params, in_dim, H, L);
  const PureTape t = carve_pure_tape(H, L, N, E, tape);
  hipError_t e;
  if ((e = gemm_linear(nf, in_dim, nullptr, nullptr, 0, nullptr, wv_rows(w.w_in, in_dim, in_dim), w.b_in, t.h[0], N, H,
                       kActTanh, nullptr, s)))
    return e;
  if (pure_train_chain(H, chain_nx, N)) {
    for (int l = 0; l < L; ++l) {
      const float *W = w.w_l + l * w.ls;
      if ((e = tgemm<VPlain, false, VPQ, false, EpiMsgTape>(
               VPlain{t.h[l], H, N, kNoSplit, 0, H}, VPQ{W, H},
               EpiMsgTape{t.h[l], t.h[l + 1], w.b_l + l * w.ls, H, chain_nx, t.m[l]}, N, 2LL * H, H, 1, s)))
        return e;
    }
    if ((e = tgemm<VPlain, false, VPlain, false, EpiTanh>(VPlain{t.h[L], H, N, kNoSplit, 0, H},
                                                           VPlain{w.w_o1, H, H, kNoSplit, 0, H},
                                                           EpiTanh{t.z, H, w.b_o1}, N, H, H, 1, s)))
      return e;
    return gemm_linear(t.z, H, nullptr, nullptr, 0, nullptr, wv_rows(w.w_o2, H, H), w.b_o2, delta, N, 3, kActNone,
                       nullptr, s);
  }
  const int *off = nullptr, *perm = nullptr;
  if (!chain_nx && L > 0) {  // by dst
    if ((e = edge_buckets(ei + E, E, N, t.buckets, s, 0, true))) return e;
    off = t.buckets.off, perm = t.buckets.perm;
  }
  float *P = t.z, *Q = t.q;  // (z itself is written after the last layer)
  for (int l = 0; l < L; ++l) {
    const float *W = w.w_l + l * w.ls;
    if ((e = gemm_linear(t.h[l], H, nullptr, nullptr, 0, nullptr, WView{W, W, 2LL * H, 1}, nullptr, P, N, H, kActNone,
                         nullptr, s)))
      return e;
    if ((e = gemm_linear(t.h[l], H, nullptr, nullptr, 0, nullptr, WView{W + H, W + H, 2LL * H, 1}, nullptr, Q, N, H,
                         kActNone, nullptr, s)))
      return e;
    hipLaunchKernelGGL(message_tape_kernel, dim3(blocks_of(N * H)), dim3(256), 0, s, t.h[l], P, Q, w.b_l + l * w.ls, ei,
                       off, perm, chain_nx, N, H, t.h[l + 1], t.m[l]);
  }
  if ((e = gemm_linear(t.h[L], H, nullptr, nullptr, 0, nullptr, wv_rows(w.w_o1, H, H), w.b_o1, t.z, N, H, kActTanh,
                       nullptr, s)))
    return e;
  return gemm_linear(t.z, H, nullptr, nullptr, 0, nullptr, wv_rows(w.w_o2, H, H), w.b_o2, delta, N, 3, kActNone,
                     nullptr, s);
}

hipError_t launch_pure_backward(const float *params, int in_dim, int H, int L, const float *nf, int64_t N,
                                const int64_t *ei, int64_t E, int chain_nx, const void *tape, const float *grad_delta,
                                float *grad_params, float *grad_nf, void *ws, hipStream_t s) {
  const PureW w = pure_view(params, in_dim, H, L);
  const PureW gv = pure_view(grad_params, in_dim, H, L);
  auto mut = [](const float *p) { return const_cast<float *>(p); };
  const PureTape t = carve_pure_tape(H, L, N, E, const_cast<void *>(tape));
  const PureBws b = carve_pure_bws(in_dim, H, L, N, E, ws);
  const bool chain = pure_train_chain(H, chain_nx, N);
  const unsigned nb = blocks_of(N * H);
  hipError_t e;
  // output_mlp.2: gW_o2 = g_delta^T z, gb_o2; a = (g_delta W_o2) * (1 - z^2)
  if ((e = gemm_wgrad(grad_delta, 3, t.z, H, N, mut(gv.w_o2), H, mut(gv.b_o2), b.gpart, s))) return e;
  hipLaunchKernelGGL(head_delta_kernel, dim3(nb), dim3(256), 0, s, grad_delta, w.w_o2, t.z, N, H, b.a);
  int cur = 0;
  if (chain) {
    const int splits = pure_wg_splits(N);
    const int S = (int)tgemm_splits(N, splits);
    // output_mlp.0: gW_o1 = a^T h_L, gb_o1 = column sums of a; g_L = a W_o1 (L = 0: times tanh'(h_0))
    if ((e = tgemm<VPlain, true, VPlain, true, EpiPart, true, true>(
             VPlain{b.a, H, N, kNoSplit, 0, H}, VPlain{t.h[L], H, N, kNoSplit, 0, H}, EpiPart{b.hpart, H, H}, H, H, N,
             splits, s, b.hbpart)))
      return e;
    {
      PrBatch pr{};
      pr.part[0] = b.hpart, pr.bpart[0] = b.hbpart, pr.gw[0] = mut(gv.w_o1), pr.gb[0] = mut(gv.b_o1);
      hipLaunchKernelGGL(pure_part_reduce_kernel, dim3(blocks_of((int64_t)H * H + H), 1), dim3(256), 0, s, pr, S, H, H, 0);
    }
    if ((e = tgemm<VPlain, false, VPlain, true, EpiGrad>(VPlain{b.a, H, N, kNoSplit, 0, H},
                                                          VPlain{w.w_o1, H, H, kNoSplit, 0, H},
                                                          EpiGrad{b.g[cur], H, nullptr, L == 0 ? t.h[0] : nullptr}, N, H, H,
                                                          1, s)))
      return e;
    for (int l = L - 1; l >= 0; --l) {
      float *gpq = b.gpq[l];
      hipLaunchKernelGGL(msg_backward_chain_kernel, dim3(nb), dim3(256), 0, s, b.g[cur], t.m[l], chain_nx, N, H, gpq,
                         gpq + H, 2LL * H);
      // g_l = g' + [gP | gQ] [W_a ; W_b]   (l = 0: times tanh'(h_0), the input layer's delta)
      if ((e = tgemm<VPlain, false, VWab, true, EpiGrad>(VPlain{gpq, 2LL * H, N, kNoSplit, 0, 2 * H},
                                                          VWab{w.w_l + l * w.ls, H},
                                                          EpiGrad{b.g[cur ^ 1], H, b.g[cur], l == 0 ? t.h[0] : nullptr},
                                                          N, H, 2LL * H, 1, s)))
        return e;
      cur ^= 1;
    }
    if (L > 0) {  // every layer's [gP | gQ]^T h_l in one launch, then one reduction of all the partials
      TgBatch<VPlain, VPlain, EpiPart> bt{};
      PrBatch pr{};
      bt.n = L;
      for (int l = 0; l < L; ++l) {
        bt.a[l] = VPlain{b.gpq[l], 2LL * H, N, kNoSplit, 0, 2 * H};
        bt.b[l] = VPlain{t.h[l], H, N, kNoSplit, 0, H};
        bt.e[l] = EpiPart{b.lpart[l], 2LL * H, H};
        bt.bias_part[l] = b.lbpart[l];
        pr.part[l] = b.lpart[l], pr.bpart[l] = b.lbpart[l];
        pr.gw[l] = mut(gv.w_l + l * gv.ls), pr.gb[l] = mut(gv.b_l + l * gv.ls);
      }
      if ((e = tgemm_batch<VPlain, VPlain, EpiPart, true>(bt, 2LL * H, H, N, splits, s))) return e;
      hipLaunchKernelGGL(pure_part_reduce_kernel, dim3(blocks_of(2LL * H * H + 2 * H), (unsigned)L), dim3(256), 0, s, pr,
                         S, 2 * H, H, 1);
    }
  } else {
    if ((e = gemm_wgrad(b.a, H, t.h[L], H, N, mut(gv.w_o1), H, mut(gv.b_o1), b.gpart, s))) return e;
    if ((e = gemm_linear(b.a, H, nullptr, nullptr, 0, nullptr, wv_t(w.w_o1, H), nullptr, b.g[cur], N, H, kActNone,
                         nullptr, s)))
      return e;
    const int *off_d = nullptr, *perm_d = nullptr, *off_s = nullptr, *perm_s = nullptr;
    if (!chain_nx && L > 0) {
      // the CSR by dst is the tape's; by src: built here
      off_d = t.buckets.off, perm_d = t.buckets.perm;
      if ((e = edge_buckets(ei, E, N, b.buckets, s))) return e;
      off_s = b.buckets.off, perm_s = b.buckets.perm;
    }
    float *gP = b.gpq[0], *gQ = b.gpq[0] + N * H;
    for (int l = L - 1; l >= 0; --l) {
      const float *W = w.w_l + l * w.ls;
      float *gW = mut(gv.w_l + l * gv.ls);
      if (chain_nx > 0)
        hipLaunchKernelGGL(msg_backward_chain_kernel, dim3(nb), dim3(256), 0, s, b.g[cur], t.m[l], chain_nx, N, H, gP, gQ,
                           (int64_t)H);
      else
        hipLaunchKernelGGL(msg_backward_csr_kernel, dim3(nb), dim3(256), 0, s, b.g[cur], t.m[l], ei + E, off_d, perm_d,
                           off_s, perm_s, N, H, gP, gQ, (int64_t)H);
      // gW_l = [gP^T h_l | gQ^T h_l], gb_l = column sums of gQ
      if ((e = gemm_wgrad(gP, H, t.h[l], H, N, gW, 2LL * H, nullptr, b.gpart, s))) return e;
      if ((e = gemm_wgrad(gQ, H, t.h[l], H, N, gW + H, 2LL * H, mut(gv.b_l + l * gv.ls), b.gpart, s))) return e;
      // g_l = g' + gP W_a + gQ W_b
      if ((e = gemm_linear(gP, H, nullptr, gQ, H, nullptr, WView{W, W + H, 1, 2LL * H}, nullptr, b.g[cur ^ 1], N, H,
                           kActNone, b.g[cur], s)))
        return e;
      cur ^= 1;
    }
    // a_0 = g_0 * (1 - h_0^2)
    hipLaunchKernelGGL(tanh_grad_kernel, dim3(nb), dim3(256), 0, s, b.g[cur], t.h[0], N * H, b.g[cur ^ 1]);
    cur ^= 1;
  }
  // input_mlp.0: gW_in = a_0^T nf, gb_in; g_nf = a_0 W_in
  const float *a0 = b.g[cur];
  if ((e = gemm_wgrad(a0, H, nf, in_dim, N, mut(gv.w_in), in_dim, mut(gv.b_in), b.gpart, s))) return e;
  if (grad_nf && (e = gemm_linear(a0, H, nullptr, nullptr, 0, nullptr, wv_t(w.w_in, in_dim), nullptr, grad_nf, N, in_dim,
                                  kActNone, nullptr, s)))
    return e;
  return hipGetLastError();
}

int64_t state_mse_ws_bytes(int B, int nx) {
  return (int64_t)carve_one<float>(mse_blocks(3LL * B * nx), nullptr).bytes;
}

hipError_t launch_state_mse(const float *delta, const float *st, const float *sn, int B, int nx, float *loss,
                            float *grad_delta, void *ws, hipStream_t s) {
  const int64_t n = 3LL * B * nx;
  const int nb = mse_blocks(n);
  float *part = carve_one<float>(nb, ws).p;
  hipLaunchKernelGGL(state_mse_kernel, dim3(nb), dim3(256), 0, s, delta, st, sn, n, nx, (float)(2.0 / (double)n), grad_delta,
                     part);
  hipLaunchKernelGGL(state_mse_final_kernel, dim3(1), dim3(256), 0, s, part, nb, (float)(1.0 / (double)n), loss);
  return hipGetLastError();
}

}  // namespace hf
