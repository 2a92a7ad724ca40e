// The k-contiguous LDS tile engine ("l16") for gfx950, shared by gemm_l16_kernel (gemm.hip) and conv_s2_l16_kernel
// (conv.hip): v_mfma_f32_16x16x4_f32 with BOTH operands kept k-contiguous in LDS.  A lane's MFMA fragment for four
// consecutive k steps is one ds_read_b128 (row i = l & 15, k = 16 kk + 4 (l >> 4) .. +3) and a staged float4 is one
// ds_write_b128 -- a quarter of the LDS instructions of the k-major 32x32x2 tile engine of mfma_gemm.h (no transposing
// ds_write_b32), and every loaded element is reused BN/32 (A) or BM/32 (B) times from registers.
// Row stride 40 floats: the 16 lanes a ds_read_b128 serves together (0-3, 12-15, 20-27 | ...) then cover all 64
// banks exactly once (i*40 + 4q mod 64 is a permutation of the 16 four-bank windows), and the 8 lanes of a
// ds_write_b128 group write 128 contiguous bytes.  One workgroup = 256 threads = 4 waves (2 x 2) = one BM x BN tile,
// BK = 32, double-buffered, one barrier per K-tile.
// The kernels keep what differs between them: tile coordinates, the stage (where a K-tile's operands come from) and
// the epilogue.  The stage is two callables (the kernels' lambdas over their own pointers and staging registers):
//   load(slot, k0)       issue the global loads of K-tile k0 into staging register set `slot` (0 .. PF-1)
//   store(slot, as, bs)  write register set `slot` to the LDS buffers as / bs (l16_lds_write)
#pragma once
#include <type_traits>

#include "dv3_common.h"
#include "mfma_gemm.h"

namespace dv3 {

constexpr int L16_BK = 32, L16_LD = 40;

// Staging map: a [rows][8] grid of float4, slot j of thread tid <-> LDS row (tid + 256 j) >> 3, k offset 4 (tid & 7).
template <int ROWS>
constexpr int l16_slots = ROWS * (L16_BK / 4) / kThreads;
__device__ __forceinline__ int l16_stage_row(int tid, int j) { return (tid + kThreads * j) >> 3; }
__device__ __forceinline__ int l16_stage_k(int tid) { return (tid & 7) * 4; }

// Where slot j of thread tid goes in an LDS buffer.  ONE_BASE spells the same row as (tid >> 3) + 32 j: one address per
// thread, the slots as immediate offsets of the ds_write_b128 (the compiler does not derive that).  The pipelined loop
// takes it; the serial loop measured slower with it on the 128 x 128 GEMM tile (profiles/r06_l16_refactor_ab.txt).
template <bool ONE_BASE>
__device__ __forceinline__ f32x4* l16_lds_slot(float* buf, int tid, int j) {
  const int row = ONE_BASE ? (tid >> 3) + (kThreads >> 3) * j : l16_stage_row(tid, j);
  return reinterpret_cast<f32x4*>(&buf[row * L16_LD + l16_stage_k(tid)]);
}
// one ds_write_b128 per staged float4; with ok: slot j is written as zeros where !ok[j]
template <bool ONE_BASE, int N>
__device__ __forceinline__ void l16_lds_write(float* buf, const f32x4 (&v)[N], int tid) {
#pragma unroll
  for (int j = 0; j < N; ++j) *l16_lds_slot<ONE_BASE>(buf, tid, j) = v[j];
}
template <bool ONE_BASE, int N>
__device__ __forceinline__ void l16_lds_write(float* buf, const f32x4 (&v)[N], const bool (&ok)[N], int tid) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < N; ++j) *l16_lds_slot<ONE_BASE>(buf, tid, j) = ok[j] ? v[j] : zero4;
}

// Accumulator map: register r of acc[a][b] in wave (wm, wn), lane (i = lane & 15, q = lane >> 4), is the tile's
// element (l16_acc_row, l16_acc_col).
template <int BM>
__device__ __forceinline__ int l16_acc_row(int wm, int a, int q, int r) { return wm * (BM / 2) + 16 * a + 4 * q + r; }
template <int BN>
__device__ __forceinline__ int l16_acc_col(int wn, int b, int i) { return wn * (BN / 2) + 16 * b + i; }

// The K loop: acc = sum over nk K-tiles, each accumulator receiving its MFMAs in ascending (t, kk, g) in either form.
// PIPELINED: software-pipelined inside the wave with two fragment sets, so that the ds_read_b128 of the next 16-k
// chunk, the ds_write_b128 of the next K-tile and the global loads of the tile after it are all issued with MFMAs of
// the same wave behind them:
//   reads (t, 1) | MFMAs (t, 0) g 0-1 | ds_write t+1 -> cur^1 | global loads t+2 | MFMAs (t, 0) g 2-3 | barrier |
//   reads (t+1, 0) | MFMAs (t, 1)
// (the barrier of t-1 came after every read of cur^1; every read of cur is complete at the barrier of t).
// Serial: read, wait, multiply per chunk; PF staging register sets, the loads of K-tile t + PF in flight while tile t
// is multiplied.  Measured (1024-row GEMM shapes): PF 2 / 4 equal PF 1 within noise -- the default; the parameter
// stays for longer-latency operands.
template <int BM, int BN, bool PIPELINED, int PF, class Load, class Store>
__device__ __forceinline__ void l16_mainloop(Load&& load, Store&& store, float (&As)[2][BM * L16_LD],
                                             float (&Bs)[2][BN * L16_LD], int wm, int wn, int lane, int nk,
                                             f32x4 (&acc)[BM / 32][BN / 32]) {
  static_assert(PF == 1 || !PIPELINED, "the pipelined loop has one staging register set");
  static_assert(BM % 32 == 0 && BN % 32 == 0 && l16_slots<BM> >= 1 && l16_slots<BN> >= 1, "tile");
  constexpr int BK = L16_BK, LD = L16_LD;
  constexpr int TM = BM / 32, TN = BN / 32;  // 16 x 16 blocks per wave (wave tile = BM/2 x BN/2)
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b) acc[a][b] = zero4;
  load(0, 0);
  store(0, As[0], Bs[0]);
#pragma unroll
  for (int u = 1; u < PF; ++u)
    if (u < nk) load(u, u * BK);
  if constexpr (PIPELINED) {
    if (nk > 1) load(0, BK);
  }
  __syncthreads();
  const int aoff = (wm * (BM / 2) + (lane & 15)) * LD + 4 * (lane >> 4);
  const int boff = (wn * (BN / 2) + (lane & 15)) * LD + 4 * (lane >> 4);
  auto fread = [&](f32x4 (&af)[TM], f32x4 (&bf)[TN], const float* as, const float* bs, int kk) {
#pragma unroll
    for (int a = 0; a < TM; ++a) af[a] = *reinterpret_cast<const f32x4*>(&as[16 * a * LD + 16 * kk]);
#pragma unroll
    for (int b = 0; b < TN; ++b) bf[b] = *reinterpret_cast<const f32x4*>(&bs[16 * b * LD + 16 * kk]);
  };
  auto mma = [&](const f32x4 (&af)[TM], const f32x4 (&bf)[TN], int g0, int g1) {
#pragma unroll
    for (int g = g0; g < g1; ++g)
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[a][g], bf[b][g], acc[a][b], 0, 0, 0);
  };
  if constexpr (PIPELINED) {
    f32x4 af[2][TM], bf[2][TN];
    fread(af[0], bf[0], As[0] + aoff, Bs[0] + boff, 0);
    // K-tiles 0 .. nk-2: tile t+1 is already in the staging registers (prologue above / the loads issued during t-1)
    for (int t = 0; t + 1 < nk; ++t) {
      const int cur = t & 1;
      fread(af[1], bf[1], As[cur] + aoff, Bs[cur] + boff, 1);
      mma(af[0], bf[0], 0, 2);
      store(0, As[cur ^ 1], Bs[cur ^ 1]);  // mid-chunk: the writes land while the second half multiplies
      if (t + 2 < nk) {
        load(0, (t + 2) * BK);
        // ISA property (check with hipcc -S): all address VALU of the block, then NA + NB global_load_dwordx4 back
        // to back, each with its own address registers.  A VALU write to the address register of a load still in the
        // issue queue waits for it; left alone the compiler threads every address through one register pair.
        __builtin_amdgcn_sched_group_barrier(0x002, 1024, 0);                           // VALU
        __builtin_amdgcn_sched_group_barrier(0x020, l16_slots<BM> + l16_slots<BN>, 0);  // VMEM read
      }
      mma(af[0], bf[0], 2, 4);
      __syncthreads();
      fread(af[0], bf[0], As[cur ^ 1] + aoff, Bs[cur ^ 1] + boff, 0);
      mma(af[1], bf[1], 0, 4);
    }
    // drain: the last K-tile (the only one when nk == 1) has nothing to stage and needs no barrier
    fread(af[1], bf[1], As[(nk - 1) & 1] + aoff, Bs[(nk - 1) & 1] + boff, 1);
    mma(af[0], bf[0], 0, 4);
    mma(af[1], bf[1], 0, 4);
  } else {
    // The fragment addresses of a tile are computed behind the tile before it, not in front of its reads: there the
    // compiler put them into the address register of the last global load just issued (same wait as above, once per
    // K-tile with the MFMAs behind it; 1.5 % of the 128 x 128 GEMM tile).  ISA property: the block after the loads
    // starts with ds_read_b128.
    const float* as = As[0] + aoff;
    const float* bs = Bs[0] + boff;
    for (int t0 = 0; t0 < nk; t0 += PF)
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int t = t0 + u;
        if (t >= nk) break;
        const int cur = t & 1;
        if (t + PF < nk) load(u, (t + PF) * BK);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          f32x4 af[TM], bf[TN];
          fread(af, bf, as, bs, kk);
          mma(af, bf, 0, 4);
        }
        if (t + 1 < nk) {
          store((u + 1) % PF, As[cur ^ 1], Bs[cur ^ 1]);
          // same property for the LDS writes: NA + NB v_add3_u32, then NA + NB ds_write_b128 back to back
          __builtin_amdgcn_sched_group_barrier(0x002, l16_slots<BM> + l16_slots<BN>, 0);  // VALU
          __builtin_amdgcn_sched_group_barrier(0x200, l16_slots<BM> + l16_slots<BN>, 0);  // DS write
        }
        as = As[cur ^ 1] + aoff;
        bs = Bs[cur ^ 1] + boff;
        __syncthreads();
      }
  }
}

// VAR of the two kernels: bit 0 the pipelined loop, bit 1 the batched epilogue.  The launchers name the VAR they ship
// and the development library's A/B switches override it: DV3_L16_LOOP (unset: as shipped, 0: the serial loop on every
// tile, 1: the pipelined loop on every tile) and DV3_L16_EPI=0 (the serial epilogue).
#ifdef DV3_DEV_SWITCHES
static inline int l16_loop_switch() { static const int loop = DV3_ENV_INT("DV3_L16_LOOP", -1); return loop; }
static inline int l16_var(int shipped) {
  static const int epi = DV3_ENV_INT("DV3_L16_EPI", 1);
  const int loop = l16_loop_switch();
  return (loop == 0 ? 0 : loop == 1 ? 1 : (shipped & 1)) | (epi ? (shipped & 2) : 0);
}
#else
constexpr int l16_var(int shipped) { return shipped; }
#endif

// f(std::integral_constant<int, l16_var(SHIPPED)>): the shipped library instantiates f for SHIPPED alone
template <int SHIPPED, class F>
static inline void l16_with_var(F&& f) {
#ifdef DV3_DEV_SWITCHES
  switch (l16_var(SHIPPED)) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 3>{});
  }
#else
  f(std::integral_constant<int, SHIPPED>{});
#endif
}

}  // namespace dv3
