// Member-batched kernels of the Plan2Explore ensemble (exploration.py:40-135 of the reference): `disag_models`
// independent MLPs (networks.MLP: [Linear(no bias) + LayerNorm + SiLU] x disag_layers + mean_layer) that all see
// the same input.  Launched member by member the ensemble is K x (layers GEMMs + layers LayerNorms + head) launches
// and a [K][M][W] prediction tensor that torch.std reads again; here every layer is ONE launch over all members
// (the member is a grid dimension) and the disagreement statistic is reduced inside the head GEMM's workgroup.
//
//   activations  [K][M][U]   (member-major; the first layer's input is ONE shared [M][F])
//   weights      [K][out][in], LayerNorm gamma / beta [K][U], head bias [K][W]  -- any member stride
//
// Built on the fp32 MFMA tile engine of mfma_gemm.h (64 x 64 x 32 tiles: widths that are no tile multiple -- the
// stock disag_units is 400 -- are handled by its edge guards).
#include "mfma_gemm.h"
#include "dv3_common.h"

namespace dv3 {

using EnsTile = TileShape<2, 2, 1, 1, 32>;  // 64 x 64, BK 32

struct EnsGemmParams {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  long lda, ldb, ldc;
  long sA, sB, sC, sBias;  // member strides in floats (sA == 0: one shared A; sC == 0: C = sum over members)
  int members, M, N, K;
  int tiles_m, tiles_n;
  int accumulate;
};

// row / column of accumulator register r of this lane inside the workgroup's 64 x 64 tile (mfma_gemm.h)
struct EnsLane {
  int wm, wn, col_l, h;
  __device__ __forceinline__ EnsLane() {
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    wm = wave / EnsTile::WN;
    wn = wave % EnsTile::WN;
    col_l = lane & 31;
    h = lane >> 5;
  }
  __device__ __forceinline__ int row(int r) const { return wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h; }
  __device__ __forceinline__ int col() const { return wn * 32 + col_l; }
};

// C_k = op(A_k) op(B_k) (+ bias_k).  TA = false: A[m][k]; TA = true: A[k][m] (weight gradients: the reduction runs
// over the rows of the batch).  TB = true: B[n][k] (y = x W^T); TB = false: B[k][n] (dx = dy W).
// sC == 0: the workgroup walks the members in ascending order and adds their tiles in registers, so the sum over
// members (the data gradient of the shared first-layer input) has a FIXED summation order and needs no atomics.
template <bool TA, bool TB>
__global__ __launch_bounds__(kThreads) void ens_gemm_kernel(EnsGemmParams p) {
  using TS = EnsTile;
  __shared__ __attribute__((aligned(16))) float lds[TS::lds_floats];
  using ATile = DenseTile<TS::BM, TS::BK, !TA>;
  using BTile = DenseTile<TS::BN, TS::BK, TB>;
  const int tiles = p.tiles_m * p.tiles_n;
  const bool reduce = (p.sC == 0);
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int wg = id % tiles;
  const int k_first = reduce ? 0 : id / tiles;
  const int k_last = reduce ? p.members : k_first + 1;
  const int m0 = (wg / p.tiles_n) * TS::BM;
  const int n0 = (wg % p.tiles_n) * TS::BN;
  const EnsLane ln;
  const int n = n0 + ln.col();

  f32x16 sum;
#pragma unroll
  for (int r = 0; r < 16; ++r) sum[r] = 0.f;
  for (int k = k_first; k < k_last; ++k) {
    DenseOperand<!TA> aop{p.A + (long)k * p.sA, nullptr, p.lda, 0, p.M, p.K, p.K, true};
    DenseOperand<TB> bop{p.B + (long)k * p.sB, nullptr, p.ldb, 0, p.N, p.K, p.K, true};
    f32x16 acc[1][1];
    bool owner;
    if (k != k_first) __syncthreads();  // the previous member's last K-tile is still being read from LDS
    mfma_mainloop<TS, ATile, BTile>(aop, bop, m0, n0, 0, p.K, lds, acc, owner);
    const float bv = (p.bias && n < p.N) ? p.bias[(long)k * p.sBias + n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] += acc[0][0][r] + bv;
  }
  if (n >= p.N) return;
  float* cbase = p.C + (long)k_first * p.sC;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + ln.row(r);
    if (m < p.M) {
      float* c = cbase + (long)m * p.ldc + n;
      *c = p.accumulate ? (*c + sum[r]) : sum[r];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// LayerNorm(eps 1e-3) + SiLU over the K*M rows of [K][M][N] with per-member gamma / beta: row r uses member r / M.
// One wave per row, the row cached in registers (N <= 64 * NV).
// ------------------------------------------------------------------------------------------------
template <int NV, bool RT = false>
__global__ __launch_bounds__(256) void ens_ln_act_fwd_kernel(const float* __restrict__ x, long ldx,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, long sG,
                                                             float* __restrict__ y, long ldy,
                                                             float* __restrict__ mean_out,
                                                             float* __restrict__ rstd_out, long R, int M, int N, int act) {
  const int l = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* g = gamma + (r / M) * sG;
  const float* b = beta + (r / M) * sG;
  const float inv_n = 1.f / (float)N;
  float xv[NV];
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = l + v * 64;
    xv[v] = (c < N) ? x[r * ldx + c] : 0.f;
    s += xv[v];
  }
  const float mean = group_sum<64>(s) * inv_n;
  float q = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const float d = (l + v * 64 < N) ? xv[v] - mean : 0.f;
    q += d * d;
  }
  const float rstd = rsqrtf(group_sum<64>(q) * inv_n + kLnEps);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = l + v * 64;
    if constexpr (RT) {
      if (c < N) y[r * ldy + c] = actf_((xv[v] - mean) * rstd * g[c] + b[c], act);
    } else {
      if (c < N) y[r * ldy + c] = siluf_((xv[v] - mean) * rstd * g[c] + b[c]);
    }
  }
  if (l == 0) {
    mean_out[r] = mean;
    rstd_out[r] = rstd;
  }
}

// dx = d(loss)/d(x) given dy = d(loss)/d(SiLU(LN(x))).  grid (row blocks, members); dgamma / dbeta [K][N] are
// ACCUMULATED (+=) with one atomicAdd per column per workgroup (the order of those adds is not fixed).
template <int NV, bool RT = false>
__global__ __launch_bounds__(256) void ens_ln_act_bwd_kernel(const float* __restrict__ dy, long lddy,
                                                             const float* __restrict__ x, long ldx,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, long sG,
                                                             const float* __restrict__ mean_in,
                                                             const float* __restrict__ rstd_in,
                                                             float* __restrict__ dx, long lddx,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                             int M, int N, int act) {
  __shared__ float red[2][64 * NV];
  const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = blockIdx.y;
  for (int c = threadIdx.x; c < 64 * NV; c += 256) {
    red[0][c] = 0.f;
    red[1][c] = 0.f;
  }
  __syncthreads();
  float g[NV], b[NV], pg[NV], pb[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = l + v * 64;
    const bool ok = c < N;
    g[v] = ok ? gamma[k * sG + c] : 0.f;
    b[v] = ok ? beta[k * sG + c] : 0.f;
    pg[v] = 0.f;
    pb[v] = 0.f;
  }
  const float inv_n = 1.f / (float)N;
  for (int mr = blockIdx.x * 4 + wave; mr < M; mr += gridDim.x * 4) {
    const long r = (long)k * M + mr;
    const float mean = mean_in[r], rstd = rstd_in[r];
    float xh[NV], dxh[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = l + v * 64;
      xh[v] = 0.f;
      dxh[v] = 0.f;
      if (c < N) {
        const float xhat = (x[r * ldx + c] - mean) * rstd;
        float dz = dy[r * lddy + c];
        if constexpr (RT) dz *= dactf_(xhat * g[v] + b[v], act);
        else dz *= dsiluf_(xhat * g[v] + b[v]);
        pg[v] += dz * xhat;
        pb[v] += dz;
        xh[v] = xhat;
        dxh[v] = dz * g[v];
        s1 += dxh[v];
        s2 += dxh[v] * xhat;
      }
    }
    s1 = group_sum<64>(s1) * inv_n;
    s2 = group_sum<64>(s2) * inv_n;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = l + v * 64;
      if (c < N) dx[r * lddx + c] = rstd * (dxh[v] - s1 - xh[v] * s2);
    }
  }
  if (dgamma) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c = l + v * 64;
      if (c < N) {
        atomicAdd(&red[0][c], pg[v]);
        atomicAdd(&red[1][c], pb[v]);
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < N; c += 256) {
      atomicAdd(dgamma + k * sG + c, red[0][c]);
      atomicAdd(dbeta + k * sG + c, red[1][c]);
    }
  }
}

// out_k[n] (+)= sum_m x_k[m][n]  (the head's bias gradient).  grid (column blocks of 64, members); the four row
// slices of a workgroup are added in a fixed order.
__global__ __launch_bounds__(256) void ens_colsum_kernel(const float* __restrict__ x, long ldx, long sX,
                                                         float* __restrict__ out, long sOut, int M, int N,
                                                         int accumulate) {
  __shared__ float red[4][64];
  const int l = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + l;
  const float* xk = x + (long)blockIdx.y * sX;
  float s = 0.f;
  if (c < N)
    for (int m = slice; m < M; m += 4) s += xk[(long)m * ldx + c];
  red[slice][l] = s;
  __syncthreads();
  if (slice == 0 && c < N) {
    const float t = ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l];
    float* o = out + (long)blockIdx.y * sOut + c;
    *o = accumulate ? (*o + t) : t;
  }
}

// ------------------------------------------------------------------------------------------------
// Ensemble regression loss (Plan2Explore._train_ensemble, exploration.py:123-133), fused with its gradient:
//   mu = tanh(pre);  loss = -1/(K M) sum_{k,m,d} log N(target[m][d]; mu_k[m][d], std)
//   dpre = d loss / d pre = (mu - target) / std^2 / (K M) * (1 - mu^2)
// The grid is fixed by the host (<= kEnsLossBlocks workgroups, grid-stride); each workgroup parks its partial sum in
// ws[block] and the last one to finish (ticket in ws[kEnsLossBlocks], reset for the next launch) adds them in block
// order: the scalar is reproducible.
// ------------------------------------------------------------------------------------------------
constexpr int kEnsLossBlocks = 1024;

__global__ __launch_bounds__(256) void ens_regress_loss_kernel(const float* pre,  // (pre and dpre may alias)
                                                               const float* __restrict__ target, long ldt,
                                                               float* dpre, float* __restrict__ loss,
                                                               float* __restrict__ ws, int members, int M, int W,
                                                               float std) {
  __shared__ float red[4];
  __shared__ int last;
  const long MW = (long)M * W, total = MW * members;
  const float inv_var = 1.f / (std * std);
  const float cst = -logf(std) - 0.91893853320467274178f;  // - log(sqrt(2 pi))
  const float wgt = 1.f / ((float)members * (float)M);
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long e = i % MW;
    const long m = e / W;
    const int d = (int)(e - m * W);
    const float mu = tanhf(pre[i]);
    const float diff = mu - target[m * ldt + d];
    s += -0.5f * diff * diff * inv_var + cst;
    dpre[i] = diff * inv_var * wgt * (1.f - mu * mu);
  }
  s = block_sum_256(s, red);
  unsigned int* ticket = reinterpret_cast<unsigned int*>(ws + kEnsLossBlocks);
  if (threadIdx.x == 0) {
    ws[blockIdx.x] = s;
    __threadfence();
    last = (atomicAdd(ticket, 1u) == gridDim.x - 1) ? 1 : 0;
  }
  __syncthreads();
  if (last && threadIdx.x == 0) {
    __threadfence();
    const volatile float* part = ws;
    float t = 0.f;
    for (unsigned int b = 0; b < gridDim.x; ++b) t += part[b];
    *loss = -t * wgt;
    *ticket = 0u;
  }
}

// ------------------------------------------------------------------------------------------------
// Disagreement (Plan2Explore._intrinsic_reward, exploration.py:108-121): the head GEMM of every member, tanh, and
// the unbiased standard deviation over the members in ONE workgroup per 64 x 64 tile of [M][W]: the workgroup walks
// the members (the head's reduction dimension is only disag_units) and keeps Welford's running mean / M2 of
// mu_k[m][d] in registers, so the [K][M][W] predictions are never read back (they are written only when the
// backward will need them: mu != nullptr).  part[tile_n][m] = sum over the tile's columns of std_k(mu_k[m][d]).
// ------------------------------------------------------------------------------------------------
struct EnsDisagParams {
  const float* h;     // [K][M][U], row stride ldh, member stride sH
  const float* w;     // [K][W][U], row stride ldw, member stride sW
  const float* bias;  // [K][W], member stride sBias
  float* mu;          // [K][M][W] contiguous or nullptr
  float* part;        // [tiles_n][M]
  long ldh, sH, ldw, sW, sBias;
  int members, M, W, U;
  int tiles_m, tiles_n;
};

__global__ __launch_bounds__(kThreads) void ens_disag_fwd_kernel(EnsDisagParams p) {
  using TS = EnsTile;
  __shared__ __attribute__((aligned(16))) float lds[TS::lds_floats];
  using ATile = DenseTile<TS::BM, TS::BK, true>;
  using BTile = DenseTile<TS::BN, TS::BK, true>;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int tm = id / p.tiles_n, tn = id % p.tiles_n;
  const int m0 = tm * TS::BM, n0 = tn * TS::BN;
  const EnsLane ln;
  const int n = n0 + ln.col();
  const bool n_ok = n < p.W;

  f32x16 mean, m2;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    mean[r] = 0.f;
    m2[r] = 0.f;
  }
  for (int k = 0; k < p.members; ++k) {
    DenseOperand<true> aop{p.h + (long)k * p.sH, nullptr, p.ldh, 0, p.M, p.U, p.U, true};
    DenseOperand<true> bop{p.w + (long)k * p.sW, nullptr, p.ldw, 0, p.W, p.U, p.U, true};
    f32x16 acc[1][1];
    bool owner;
    if (k) __syncthreads();
    mfma_mainloop<TS, ATile, BTile>(aop, bop, m0, n0, 0, p.U, lds, acc, owner);
    const float bv = n_ok ? p.bias[(long)k * p.sBias + n] : 0.f;
    const float inv_cnt = 1.f / (float)(k + 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = tanhf(acc[0][0][r] + bv);
      const float d = v - mean[r];
      mean[r] += d * inv_cnt;
      m2[r] += d * (v - mean[r]);
      if (p.mu) {
        const int m = m0 + ln.row(r);
        if (n_ok && m < p.M) p.mu[((long)k * p.M + m) * p.W + n] = v;
      }
    }
  }
  // row sums of the tile's standard deviations: 32 columns of a wave by shuffles, the two column waves through LDS
  const float inv_km1 = 1.f / (float)(p.members - 1);
  float rs[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) rs[r] = group_sum<32>(n_ok ? sqrtf(fmaxf(m2[r], 0.f) * inv_km1) : 0.f);
  __syncthreads();
  if (ln.wn == 1 && ln.col_l == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) lds[ln.row(r)] = rs[r];
  }
  __syncthreads();
  if (ln.wn == 0 && ln.col_l == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + ln.row(r);
      if (m < p.M) p.part[(long)tn * p.M + m] = rs[r] + lds[ln.row(r)];
    }
  }
}

// disag[m] = (sum_tn part[tn][m]) / W;  reward[m] = scale * (log ? log(disag) : disag)
__global__ __launch_bounds__(256) void ens_disag_finish_kernel(const float* __restrict__ part, int tiles_n,
                                                               float* __restrict__ disag,
                                                               float* __restrict__ reward, long ldr, int M, int W,
                                                               float scale, int use_log) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float s = 0.f;
  for (int t = 0; t < tiles_n; ++t) s += part[(long)t * M + m];
  s /= (float)W;
  disag[m] = s;
  reward[(long)m * ldr] = scale * (use_log ? logf(s) : s);
}

// mu [K][M][W] -> d reward-objective / d pre_k, in place:
//   g[m] = dreward[m] * scale * (log ? 1 / disag[m] : 1) / W
//   d std / d mu_k = (mu_k - mean) / ((K - 1) std);   dpre_k = g * that * (1 - mu_k^2)
// One thread per (m, d): a Welford pass over the members, then the write pass.
__global__ __launch_bounds__(256) void ens_disag_bwd_kernel(float* __restrict__ mu, const float* __restrict__ disag,
                                                            const float* __restrict__ dreward, long lddr,
                                                            int members, int M, int W, float scale, int use_log) {
  const long MW = (long)M * W;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= MW) return;
  const long m = e / W;
  float mean = 0.f, m2 = 0.f;
  for (int k = 0; k < members; ++k) {
    const float v = mu[k * MW + e];
    const float d = v - mean;
    mean += d / (float)(k + 1);
    m2 += d * (v - mean);
  }
  const float km1 = (float)(members - 1);
  const float sd = sqrtf(m2 / km1);
  float g = dreward[m * lddr] * scale / (float)W;
  if (use_log) g /= disag[m];
  const float f = (sd > 0.f) ? g / (km1 * sd) : 0.f;
  for (int k = 0; k < members; ++k) {
    const float v = mu[k * MW + e];
    mu[k * MW + e] = f * (v - mean) * (1.f - v * v);
  }
}

// ------------------------------------------------------------------------------------------------
// Row packing: dst[m][off_i : off_i + w_i] = src_i[m][:] for up to three row-strided sources, off_i = the running sum
// of the widths (the ensemble's shared input [stoch | deter | action] and its regression target, assembled from
// slices of the posterior / the imagined trajectory in ONE launch).  Flat over M * (units per row): a source whose
// rows can be moved as 16-byte vectors (base, row strides, width and destination offset all multiples of 4 floats:
// decided by the host, vec[i]) contributes w_i / 4 units per row, any other source w_i dword units.
// ------------------------------------------------------------------------------------------------
struct EnsPackParams {
  const float* src[3];
  long ld[3];
  int off[3];    // first destination column of source i
  int units[3];  // units per row of source i (0: absent)
  int vec[3];
  float* dst;
  long ld_dst;
  long total;  // M * U
  int U;       // units per row, all sources
};

__global__ __launch_bounds__(256) void ens_pack_rows_kernel(EnsPackParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const long m = i / p.U;
  int u = (int)(i - m * p.U);
  int s = 0;
  if (u >= p.units[0]) {
    u -= p.units[0];
    s = 1;
    if (u >= p.units[1]) {
      u -= p.units[1];
      s = 2;
    }
  }
  const float* src = p.src[s] + m * p.ld[s];
  float* dst = p.dst + m * p.ld_dst + p.off[s];
  if (p.vec[s])
    reinterpret_cast<float4*>(dst)[u] = reinterpret_cast<const float4*>(src)[u];
  else
    dst[u] = src[u];
}

static bool fits_int(long v) { return v >= 0 && v <= 0x7fffffffL; }

}  // namespace dv3

using namespace dv3;

extern "C" int dv3_ens_gemm_f32(int members, int transA, int transB, int M, int N, int K, const float* A, long lda,
                                long strideA, const float* B, long ldb, long strideB, float* C, long ldc,
                                long strideC, const float* bias, long strideBias, int accumulate, void* stream) {
  if (members <= 0 || M <= 0 || N <= 0) return 0;
  if (K <= 0 || !A || !B || !C || strideA < 0 || strideB < 0 || strideC < 0 || strideBias < 0) return DV3_ERR_ARG;
  if (lda < (transA ? M : K) || ldb < (transB ? K : N) || ldc < N) return DV3_ERR_ARG;
  if (transA && transB) return DV3_ERR_ARG;
  EnsGemmParams p{};
  p.A = A; p.B = B; p.C = C; p.bias = bias;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.sA = strideA; p.sB = strideB; p.sC = strideC; p.sBias = strideBias;
  p.members = members; p.M = M; p.N = N; p.K = K;
  p.tiles_m = (M + EnsTile::BM - 1) / EnsTile::BM;
  p.tiles_n = (N + EnsTile::BN - 1) / EnsTile::BN;
  p.accumulate = accumulate ? 1 : 0;
  const long grid = (long)p.tiles_m * p.tiles_n * (strideC == 0 ? 1 : members);
  if (!fits_int(grid)) return DV3_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  dim3 g((unsigned)grid), b(kThreads);
  if (!transA && transB) hipLaunchKernelGGL((ens_gemm_kernel<false, true>), g, b, 0, s, p);
  else if (!transA && !transB) hipLaunchKernelGGL((ens_gemm_kernel<false, false>), g, b, 0, s, p);
  else hipLaunchKernelGGL((ens_gemm_kernel<true, false>), g, b, 0, s, p);
  return (int)hipGetLastError();
}

#define DV3_ENS_NV_DISPATCH(KERNEL, RT_, GRID, ...)                                                      \
  do {                                                                                                 \
    if (N <= 64) hipLaunchKernelGGL((KERNEL<1, RT_>), GRID, dim3(256), 0, s, __VA_ARGS__);                  \
    else if (N <= 128) hipLaunchKernelGGL((KERNEL<2, RT_>), GRID, dim3(256), 0, s, __VA_ARGS__);            \
    else if (N <= 256) hipLaunchKernelGGL((KERNEL<4, RT_>), GRID, dim3(256), 0, s, __VA_ARGS__);            \
    else if (N <= 512) hipLaunchKernelGGL((KERNEL<8, RT_>), GRID, dim3(256), 0, s, __VA_ARGS__);            \
    else if (N <= 1024) hipLaunchKernelGGL((KERNEL<16, RT_>), GRID, dim3(256), 0, s, __VA_ARGS__);          \
    else hipLaunchKernelGGL((KERNEL<32, RT_>), GRID, dim3(256), 0, s, __VA_ARGS__);                         \
  } while (0)

extern "C" int dv3_ens_ln_act_fwd_ex(const float* x, long ldx, const float* gamma, const float* beta, long strideG,
                                     float* y, long ldy, float* mean, float* rstd, int members, int M, int N, int act,
                                     void* stream) {
  if (!dv3_act_ok(act)) return DV3_ERR_ARG;
  if (members <= 0 || M <= 0) return 0;
  if (!x || !gamma || !beta || !y || !mean || !rstd || N <= 0 || N > 2048 || ldx < N || ldy < N || strideG < 0)
    return DV3_ERR_ARG;
  const long R = (long)members * M;
  const long blocks = (R + 3) / 4;
  if (!fits_int(blocks)) return DV3_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (act != DV3_ACT_SILU)  // (code 0 too: the SiLU instantiation has no switch)
    DV3_ENS_NV_DISPATCH(ens_ln_act_fwd_kernel, true, dim3((unsigned)blocks), x, ldx, gamma, beta, strideG, y, ldy, mean,
                        rstd, R, M, N, act);
  else
    DV3_ENS_NV_DISPATCH(ens_ln_act_fwd_kernel, false, dim3((unsigned)blocks), x, ldx, gamma, beta, strideG, y, ldy, mean,
                        rstd, R, M, N, act);
  return (int)hipGetLastError();
}

extern "C" int dv3_ens_ln_act_fwd(const float* x, long ldx, const float* gamma, const float* beta, long strideG,
                                  float* y, long ldy, float* mean, float* rstd, int members, int M, int N,
                                  void* stream) {
  return dv3_ens_ln_act_fwd_ex(x, ldx, gamma, beta, strideG, y, ldy, mean, rstd, members, M, N, DV3_ACT_SILU, stream);
}

extern "C" int dv3_ens_ln_act_bwd_ex(const float* dy, long lddy, const float* x, long ldx, const float* gamma,
                                     const float* beta, long strideG, const float* mean, const float* rstd, float* dx,
                                     long lddx, float* dgamma, float* dbeta, int members, int M, int N, int act,
                                     void* stream) {
  if (!dv3_act_ok(act)) return DV3_ERR_ARG;
  if (members <= 0 || M <= 0) return 0;
  if (!dy || !x || !gamma || !beta || !mean || !rstd || !dx || N <= 0 || N > 2048 || lddy < N || ldx < N ||
      lddx < N || strideG < 0 || members > 65535 || (dgamma == nullptr) != (dbeta == nullptr))
    return DV3_ERR_ARG;
  int bx = (M + 3) / 4;
  if (bx > 64) bx = 64;
  hipStream_t s = (hipStream_t)stream;
  if (act != DV3_ACT_SILU)
    DV3_ENS_NV_DISPATCH(ens_ln_act_bwd_kernel, true, dim3((unsigned)bx, (unsigned)members), dy, lddy, x, ldx, gamma, beta,
                        strideG, mean, rstd, dx, lddx, dgamma, dbeta, M, N, act);
  else
    DV3_ENS_NV_DISPATCH(ens_ln_act_bwd_kernel, false, dim3((unsigned)bx, (unsigned)members), dy, lddy, x, ldx, gamma, beta,
                        strideG, mean, rstd, dx, lddx, dgamma, dbeta, M, N, act);
  return (int)hipGetLastError();
}

extern "C" int dv3_ens_ln_act_bwd(const float* dy, long lddy, const float* x, long ldx, const float* gamma,
                                  const float* beta, long strideG, const float* mean, const float* rstd, float* dx,
                                  long lddx, float* dgamma, float* dbeta, int members, int M, int N, void* stream) {
  return dv3_ens_ln_act_bwd_ex(dy, lddy, x, ldx, gamma, beta, strideG, mean, rstd, dx, lddx, dgamma, dbeta, members, M, N,
                               DV3_ACT_SILU, stream);
}

extern "C" int dv3_ens_colsum(const float* x, long ldx, long strideX, float* out, long strideOut, int members, int M,
                              int N, int accumulate, void* stream) {
  if (members <= 0 || N <= 0) return 0;
  if (!x || !out || M <= 0 || ldx < N || strideX < 0 || strideOut < 0 || members > 65535) return DV3_ERR_ARG;
  hipLaunchKernelGGL(ens_colsum_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)members), dim3(256), 0,
                     (hipStream_t)stream, x, ldx, strideX, out, strideOut, M, N, accumulate ? 1 : 0);
  return (int)hipGetLastError();
}

extern "C" int dv3_ens_regress_loss(const float* pre, const float* target, long ldt, float* dpre, float* loss,
                                    float* ws, int members, int M, int W, float std, void* stream) {
  if (!pre || !target || !dpre || !loss || !ws || members <= 0 || M <= 0 || W <= 0 || ldt < W || !(std > 0.f))
    return DV3_ERR_ARG;
  const long total = (long)members * M * W;
  long blocks = (total + 255) / 256;
  if (blocks > kEnsLossBlocks) blocks = kEnsLossBlocks;
  hipLaunchKernelGGL(ens_regress_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pre, target,
                     ldt, dpre, loss, ws, members, M, W, std);
  return (int)hipGetLastError();
}

extern "C" int dv3_ens_disag_fwd(const float* h, long ldh, long strideH, const float* w, long ldw, long strideW,
                                 const float* bias, long strideBias, float* mu, float* part, float* disag,
                                 float* reward, long ldr, int members, int M, int W, int U, float scale, int use_log,
                                 void* stream) {
  if (members < 2) return DV3_ERR_ARG;  // the unbiased std over members needs two of them
  if (!h || !w || !bias || !part || !disag || !reward || M <= 0 || W <= 0 || U <= 0 || ldh < U || ldw < U ||
      ldr < 1 || strideH < 0 || strideW < 0 || strideBias < 0)
    return DV3_ERR_ARG;
  EnsDisagParams p{};
  p.h = h; p.w = w; p.bias = bias; p.mu = mu; p.part = part;
  p.ldh = ldh; p.sH = strideH; p.ldw = ldw; p.sW = strideW; p.sBias = strideBias;
  p.members = members; p.M = M; p.W = W; p.U = U;
  p.tiles_m = (M + EnsTile::BM - 1) / EnsTile::BM;
  p.tiles_n = (W + EnsTile::BN - 1) / EnsTile::BN;
  const long grid = (long)p.tiles_m * p.tiles_n;
  if (!fits_int(grid)) return DV3_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ens_disag_fwd_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, p);
  hipLaunchKernelGGL(ens_disag_finish_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, part, p.tiles_n,
                     disag, reward, ldr, M, W, scale, use_log ? 1 : 0);
  return (int)hipGetLastError();
}

extern "C" int dv3_ens_disag_bwd(float* mu, const float* disag, const float* dreward, long lddr, int members, int M,
                                 int W, float scale, int use_log, void* stream) {
  if (members < 2) return DV3_ERR_ARG;
  if (!mu || !disag || !dreward || M <= 0 || W <= 0 || lddr < 1) return DV3_ERR_ARG;
  const long blocks = ((long)M * W + 255) / 256;
  if (!fits_int(blocks)) return DV3_ERR_ARG;
  hipLaunchKernelGGL(ens_disag_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mu, disag,
                     dreward, lddr, members, M, W, scale, use_log ? 1 : 0);
  return (int)hipGetLastError();
}

static bool aligned16(const void* q) { return (reinterpret_cast<unsigned long long>(q) & 15ull) == 0; }

extern "C" int dv3_ens_pack_rows(const float* src0, long ld0, int w0, const float* src1, long ld1, int w1,
                                 const float* src2, long ld2, int w2, float* dst, long ld_dst, long M, void* stream) {
  const float* src[3] = {src0, src1, src2};
  const long ld[3] = {ld0, ld1, ld2};
  const int w[3] = {w0, w1, w2};
  if (M < 0 || w0 < 0 || w1 < 0 || w2 < 0) return DV3_ERR_ARG;
  const long W = (long)w0 + w1 + w2;
  if (!fits_int(W)) return DV3_ERR_ARG;
  for (int i = 0; i < 3; ++i)
    if (w[i] > 0 && (!src[i] || ld[i] < w[i])) return DV3_ERR_ARG;
  if (W > 0 && (!dst || ld_dst < W)) return DV3_ERR_ARG;
  if (M == 0 || W == 0) return 0;
  EnsPackParams p{};
  p.dst = dst;
  p.ld_dst = ld_dst;
  int off = 0, U = 0;
  for (int i = 0; i < 3; ++i) {
    p.src[i] = src[i];
    p.ld[i] = ld[i];
    p.off[i] = off;
    p.vec[i] = (w[i] > 0 && w[i] % 4 == 0 && off % 4 == 0 && ld[i] % 4 == 0 && ld_dst % 4 == 0 && aligned16(src[i]) &&
                aligned16(dst))
                   ? 1
                   : 0;
    p.units[i] = p.vec[i] ? w[i] / 4 : w[i];
    U += p.units[i];
    off += w[i];
  }
  p.U = U;
  p.total = M * (long)U;
  const long blocks = (p.total + 255) / 256;
  if (M > 0x7fffffffL || !fits_int(blocks)) return DV3_ERR_ARG;
  hipLaunchKernelGGL(ens_pack_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}
