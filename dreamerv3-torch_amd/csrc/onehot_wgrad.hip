// Weight gradient of a Linear over an exact one-hot input: gW[u][s*D + d] += sum over the rows m with idx[m][s] == d
// of dY[m][u]  (= dY^T @ onehot(idx), the stoch columns of every layer that reads feat = [stoch | deter]:
// networks.py:154-159, tools.py:452-460).  A segment sum: R*S*U additions where the dense TN product spends R*S*D*U
// multiply-adds, D - 1 of every D against 0.0 (1/32 of the work at D = 32), and no one-hot operand to stream.
//
// Stage 1 (onehot_wgrad_sum_kernel): a workgroup owns 32 columns of dY, all S groups and one split of the rows, and
// keeps the [S*D][32] accumulator tile in LDS (128 KiB at S*D = 1024: one workgroup per CU).  16 lanes own one group:
// a lane owns 2 columns of that group's D accumulator rows for the whole launch, so no two lanes ever touch the same
// accumulator -- no atomics, no barrier in the row loop (ds_add_f32 runs at ~2 lanes/clk).  Per row a
// lane reads its 8 bytes of dY once and does one 8-byte LDS read-add-write.  The rows of groups s and s+1 interleave
// in the tile, so the two groups a 32-lane LDS cycle serves fall into complementary bank halves whatever their
// classes are: ds_read_b64 / ds_write_b64 run conflict-free at 256 B/clk.  Rows are taken four at a time: the four
// reads are issued together and a later row that hits the class of an earlier one takes the earlier row's sum instead
// of its (stale) read, so the adds of an accumulator still happen in row order -- the result does not depend on the
// batching -- while one LDS round trip covers four rows.  A row's class indices reach the lanes of a group as one
// 4-byte load per 4 rows and a quad broadcast.  The whole tile, untouched classes included, goes to the partials
// buffer: nothing needs clearing.
// Stage 2 (onehot_wgrad_reduce_kernel): gW += the partials in ascending split order, transposed to [U][ldw] through
// a 32 x 32 LDS tile.  Fixed order everywhere: two launches on the same inputs give the same bits.
#include "dv3_common.h"

namespace dv3 {

constexpr int kOwCols = 32;  // dY columns per workgroup (tile row = 32 floats: one 32-bank half per group)

struct OWParams {
  const float* dY;  // [R][ldy]
  long ldy;
  const int* idx;  // [R][S]
  long R;
  int U, S, D;
  float* part;  // [nsplit][ncb][S*D][32]
  int nsplit;
  long rows_per_split;
};

// tile row of (group s, class d): groups pair up so that s and s+1 sit in complementary bank halves
__device__ __forceinline__ int ow_tile_row(int s, int d, int D) { return (((s >> 1) * D + d) << 1) | (s & 1); }

// 8 rows of this lane's operands: its 2 columns of dY, and the class indices of its group for rows 0-3 and 4-7 -- lane
// j of every 4 lanes holds row j's (ip points at this lane's own row and group), handed round by a quad broadcast
struct OwBatch {
  float2 v[8];
  int ia, ib;
};

__device__ __forceinline__ void ow_load(OwBatch& b, const float* __restrict__ dy, long ldy,
                                        const int* __restrict__ ip, int S) {
#pragma unroll
  for (int j = 0; j < 8; ++j) b.v[j] = *reinterpret_cast<const float2*>(dy + j * ldy);
  b.ia = ip[0];
  b.ib = ip[4 * (long)S];
}

template <int J>
__device__ __forceinline__ int ow_quad_bcast(int x) {
  return __builtin_amdgcn_mov_dpp(x, J | (J << 2) | (J << 4) | (J << 6), 0xf, 0xf, true);
}

// 4 rows into the tile: v -> their dY values, i4 = the quad's four class indices
__device__ __forceinline__ void ow_add4(float* __restrict__ acc, const float2* v, int i4, int dmax, int rowbase) {
  int a[4];
  float2 n[4];
  const int d4[4] = {ow_quad_bcast<0>(i4), ow_quad_bcast<1>(i4), ow_quad_bcast<2>(i4), ow_quad_bcast<3>(i4)};
#pragma unroll
  for (int j = 0; j < 4; ++j)  // (an index out of range must not leave the tile)
    a[j] = rowbase + (int)min((unsigned)d4[j], (unsigned)dmax) * (2 * kOwCols);
#pragma unroll
  for (int j = 0; j < 4; ++j) n[j] = *reinterpret_cast<const float2*>(acc + a[j]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int k = 0; k < j; ++k)
      if (a[k] == a[j]) n[j] = n[k];  // (ascending k: the latest earlier row of this class wins)
    n[j].x += v[j].x;
    n[j].y += v[j].y;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) *reinterpret_cast<float2*>(acc + a[j]) = n[j];  // (in order: the last row's sum stays)
}

__global__ __launch_bounds__(1024) void onehot_wgrad_sum_kernel(OWParams p) {
  extern __shared__ float ow_acc[];  // [S*D][32]
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int tile = p.S * p.D * kOwCols;
  for (int i = tid * 4; i < tile; i += nthr * 4) *reinterpret_cast<float4*>(ow_acc + i) = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  const int cb = blockIdx.x, split = blockIdx.y;
  const int s = tid >> 4, cp = tid & 15;  // s < S: the block has 16 S threads
  const int u = cb * kOwCols + 2 * cp;
  // a lane past the last column (U is even: a pair is in or out as a whole) sums columns 0, 1 into tile columns that
  // stage 2 never reads
  const bool live = u < p.U;
  const int rowbase = ow_tile_row(s, 0, p.D) * kOwCols + 2 * cp;
  const long r0 = (long)split * p.rows_per_split;
  const long r1 = min(p.R, r0 + p.rows_per_split);
  const float* dy = p.dY + r0 * p.ldy + (live ? u : 0);
  const long ldy = p.ldy;
  const int S = p.S, dmax = p.D - 1;
  const int* ip = p.idx + r0 * S + s;
  long m = r0;
  // 8 rows per step, their operands loaded one step ahead (two waves per SIMD do not hide a memory round trip)
  if (m + 8 <= r1) {
    const long quad_row = (long)(cp & 3) * S;
    OwBatch cur;
    ow_load(cur, dy, ldy, ip + quad_row, S);
    for (; m + 16 <= r1; m += 8) {
      dy += 8 * ldy, ip += 8 * (long)S;
      OwBatch nxt;
      ow_load(nxt, dy, ldy, ip + quad_row, S);
      ow_add4(ow_acc, cur.v, cur.ia, dmax, rowbase);
      ow_add4(ow_acc, cur.v + 4, cur.ib, dmax, rowbase);
      cur = nxt;
    }
    ow_add4(ow_acc, cur.v, cur.ia, dmax, rowbase);
    ow_add4(ow_acc, cur.v + 4, cur.ib, dmax, rowbase);
    m += 8, dy += 8 * ldy, ip += 8 * (long)S;
  }
  for (; m < r1; ++m, dy += ldy, ip += S) {
    const float2 v = *reinterpret_cast<const float2*>(dy);
    const int d = (int)min((unsigned)ip[0], (unsigned)dmax);
    float2* q = reinterpret_cast<float2*>(ow_acc + rowbase + d * (2 * kOwCols));
    float2 n = *q;
    n.x += v.x;
    n.y += v.y;
    *q = n;
  }
  __syncthreads();
  float* out = p.part + ((long)split * gridDim.x + cb) * tile;
  for (int i = tid * 4; i < tile; i += nthr * 4) *reinterpret_cast<float4*>(out + i) = *reinterpret_cast<const float4*>(ow_acc + i);
}

// gW[u][k] += sum over the splits (ascending) of part[split][u / 32][tile row of k][u % 32]; one 32 (u) x 32 (k) tile
// per workgroup, read along u and written along k.
__global__ __launch_bounds__(256) void onehot_wgrad_reduce_kernel(const float* __restrict__ part, int nsplit, int ncb,
                                                                  int U, int S, int D, float* __restrict__ gW, long ldw) {
  __shared__ float t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int SD = S * D;
  const int k0 = blockIdx.x * 32, cb = blockIdx.y;
  const long tile = (long)SD * kOwCols;
#pragma unroll
  for (int j = 0; j < 32; j += 8) {
    const int k = k0 + ty + j;
    float sum = 0.f;
    if (k < SD) {
      const float* q = part + (long)cb * tile + (long)ow_tile_row(k / D, k % D, D) * kOwCols + tx;
      for (int sp = 0; sp < nsplit; ++sp) sum += q[(long)sp * ncb * tile];
    }
    t[ty + j][tx] = sum;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 32; j += 8) {
    const int u = cb * kOwCols + ty + j, k = k0 + tx;
    if (u < U && k < SD) gW[(long)u * ldw + k] += t[tx][ty + j];
  }
}

}  // namespace dv3

using namespace dv3;

// floats of partials a launch with `nsplit` row splits writes
static long ow_partials(int U, int S, int D, int nsplit) {
  return (long)nsplit * ((U + kOwCols - 1) / kOwCols) * S * D * kOwCols;
}

extern "C" int dv3_onehot_wgrad(const float* dY, long ldy, const int* idx, long R, int U, int S, int D, float* gW,
                                long ldw, float* partials, long partials_floats, int nsplit, void* stream) {
  if (R <= 0 || U == 0) return 0;
  if (!dY || !idx || !gW || !partials || U < 0 || (U & 1) || (ldy & 1) || ldy < U || ((uintptr_t)dY & 7) || ((uintptr_t)idx & 3) ||
      ((uintptr_t)partials & 15) || S <= 0 || (S & 3) || S > 64 || D <= 0 || (long)S * D > 1024 || ldw < (long)S * D ||
      nsplit <= 0 || nsplit > R || nsplit > 65535)
    return DV3_ERR_ARG;
  const int ncb = (U + kOwCols - 1) / kOwCols;
  if (partials_floats < ow_partials(U, S, D, nsplit)) return DV3_ERR_ARG;
  const long rows_per_split = (R + nsplit - 1) / nsplit;
  nsplit = (int)((R + rows_per_split - 1) / rows_per_split);  // (the last split may be ragged, never empty)
  const int SD = S * D;
  const size_t lds = (size_t)SD * kOwCols * sizeof(float);
  static unsigned long long seen[4];
  if (lds > 64 * 1024 && dv3_first_on_device(seen)) {
    if (hipFuncSetAttribute((const void*)onehot_wgrad_sum_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            128 * 1024) != hipSuccess)
      return (int)hipGetLastError();
  }
  OWParams p{dY, ldy, idx, R, U, S, D, partials, nsplit, rows_per_split};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(onehot_wgrad_sum_kernel, dim3(ncb, nsplit), dim3(16 * S), lds, s, p);
  hipLaunchKernelGGL(onehot_wgrad_reduce_kernel, dim3((SD + 31) / 32, ncb), dim3(256), 0, s, partials, nsplit, ncb, U, S,
                     D, gW, ldw);
  return (int)hipGetLastError();
}
