// Continuous (diagonal Gaussian) latents, dyn_discrete: 0: the stat-layer head with its reparameterised
// sample, its backward, and the KL / entropies with their backward.  Reference: RSSM._suff_stats_layer
// (networks.py:251-270), RSSM.get_dist (networks.py:167-171) with tools.ContDist.sample / .mode
// (tools.py:586-599), RSSM.kl_loss (networks.py:272-290) over torch.distributions.kl._kl_normal_normal.
//
// Rows are short (S = 8..64 in practice, S <= 1024).  The head and both backward kernels are element-wise, so they
// run flat over the M*S elements (consecutive lanes take consecutive elements across row boundaries: several rows
// per wavefront when S is small).  The KL forward reduces a row inside a group of G = pow2 >= min(S, 64)
// consecutive lanes, 64/G rows per wavefront.
#include "dv3_common.h"

namespace dv3 {

enum { kMeanNone = 0, kMeanTanh5 = 1 };
// kStdIdentity: std_raw already is the standard deviation (sampling from the {mean, std} _suff_stats_layer returned)
enum { kStdSoftplus = 0, kStdAbs = 1, kStdSigmoid = 2, kStdSigmoid2 = 3, kStdIdentity = 4 };

constexpr float kHalfLog2PiPlusHalf = 1.4189385332046727f;  // 1/2 + 1/2 ln(2 pi)

// mean activation and its derivative (networks.py:259-262)
__device__ __forceinline__ float mean_act_f(float x, int act, float& d) {
  if (act == kMeanTanh5) {
    const float t = tanhf(x * 0.2f);
    d = 1.f - t * t;
    return 5.f * t;
  }
  d = 1.f;
  return x;
}

// std activation (before + min_std) and its derivative (networks.py:263-268)
__device__ __forceinline__ float std_act_f(float x, int act, float& d) {
  switch (act) {
    case kStdSoftplus: {  // torch softplus, beta 1, threshold 20
      d = sigmoidf_(x);
      if (x > 20.f) {
        d = 1.f;
        return x;
      }
      return log1pf(expf(x));
    }
    case kStdAbs: {
      const float v = x + 1.f;
      d = (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f);
      return fabsf(v);
    }
    case kStdSigmoid: {
      const float s = sigmoidf_(x);
      d = s * (1.f - s);
      return s;
    }
    case kStdSigmoid2: {  // 2 sigmoid(x / 2)
      const float s = sigmoidf_(0.5f * x);
      d = s * (1.f - s);
      return 2.f * s;
    }
    default:
      d = 1.f;
      return x;
  }
}

// element e of the N(0,1) stream fill_normal_kernel (optim.hip) writes at the same offset.  One Philox block per
// element, i.e. four times the blocks fill_normal_kernel computes: the flat mapping keeps every lane on its own
// element, and at these sizes (M S <= a few thousand in the scans) the launch is at its fixed cost either way.
__device__ __forceinline__ float philox_normal(unsigned long long seed, unsigned long long offset,
                                               unsigned long long e) {
  uint32_t o[4];
  Philox ph(seed);
  ph(offset + (e >> 2), 0x6e6f726dULL, o);
  const int j = (int)(e & 3);
  const float rad = sqrtf(-2.f * logf(u01(o[j & 2])));
  const float ang = 6.283185307179586f * u01(o[(j & 2) + 1]);
  return (j & 1) ? rad * sinf(ang) : rad * cosf(ang);
}

// raw [M, 2S] = mean_raw | std_raw  ->  mean, std, stoch = mean + std eps (mode: stoch = mean), all [M, S].
// nb_*: the next observe step's reset blend of the sample, next_out = stoch (1 - first[m]) + init[s] first[m].
__global__ __launch_bounds__(256) void gauss_head_fwd_kernel(const float* __restrict__ raw,
                                                             const float* __restrict__ eps,
                                                             const unsigned long long* __restrict__ rng_state,
                                                             unsigned long long offset_add,
                                                             float* __restrict__ eps_out, float* __restrict__ mean,
                                                             float* __restrict__ stdv, float* __restrict__ stoch,
                                                             long M, int S, int mean_act, int std_act, float min_std,
                                                             int mode, const float* __restrict__ nb_first,
                                                             const float* __restrict__ nb_init,
                                                             float* __restrict__ nb_out) {
  unsigned long long seed = 0, offset = 0;
  const bool draw = !mode && !eps;
  if (draw) {
    seed = rng_state[0];
    offset = rng_state[1] + offset_add;
  }
  const long total = M * S;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long m = e / S;
    const int s = (int)(e - m * S);
    float dm, ds;
    const float mu = mean_act_f(raw[m * 2 * S + s], mean_act, dm);
    const float sd = std_act_f(raw[m * 2 * S + S + s], std_act, ds) + min_std;
    float v = mu;
    if (!mode) {
      const float z = draw ? philox_normal(seed, offset, (unsigned long long)e) : eps[e];
      if (eps_out) eps_out[e] = z;
      v = mu + sd * z;
    }
    if (mean) mean[e] = mu;
    if (stdv) stdv[e] = sd;
    stoch[e] = v;
    if (nb_out) {
      const float f = nb_first[m];
      nb_out[e] = v * (1.f - f) + nb_init[s] * f;
    }
  }
}

// d mean_raw = (dstoch + dmean) mean_act',  d std_raw = (dstoch eps + dstd) std_act'   (no eps term in mode form)
__global__ __launch_bounds__(256) void gauss_head_bwd_kernel(const float* __restrict__ dstoch,
                                                             const float* __restrict__ dmean,
                                                             const float* __restrict__ dstd,
                                                             const float* __restrict__ raw,
                                                             const float* __restrict__ eps, float* __restrict__ draw,
                                                             long M, int S, int mean_act, int std_act, int mode,
                                                             int accumulate) {
  const long total = M * S;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long m = e / S;
    const int s = (int)(e - m * S);
    const long im = m * 2 * S + s, is = im + S;
    float dm, ds;
    mean_act_f(raw[im], mean_act, dm);
    std_act_f(raw[is], std_act, ds);
    const float g = dstoch ? dstoch[e] : 0.f;
    float gm = g, gs = 0.f;
    if (!mode && dstoch) gs = g * eps[e];
    if (dmean) gm += dmean[e];
    if (dstd) gs += dstd[e];
    gm *= dm;
    gs *= ds;
    draw[im] = accumulate ? draw[im] + gm : gm;
    draw[is] = accumulate ? draw[is] + gs : gs;
  }
}

// kl[r] = sum_s ( 1/2 ((s1/s2)^2 + ((m1-m2)/s2)^2 - 1) - ln(s1/s2) ),  ent = sum_s (1/2 + 1/2 ln 2 pi + ln sigma)
template <int G>
__global__ __launch_bounds__(256) void gauss_kl_fwd_kernel(const float* __restrict__ m1, const float* __restrict__ s1,
                                                           const float* __restrict__ m2, const float* __restrict__ s2,
                                                           float* __restrict__ kl, float* __restrict__ ent_post,
                                                           float* __restrict__ ent_prior, long R, int S) {
  constexpr int RPB = 256 / G;
  const int sub = threadIdx.x / G, l = threadIdx.x % G;
  for (long r0 = (long)blockIdx.x * RPB; r0 < R; r0 += (long)gridDim.x * RPB) {
    const long r = r0 + sub;
    const bool rv = r < R;
    float a_kl = 0.f, a_ep = 0.f, a_eq = 0.f;
    if (rv) {
      for (int s = l; s < S; s += G) {
        const long e = r * S + s;
        const float p = s1[e], q = s2[e];
        const float ratio = p / q, d = (m1[e] - m2[e]) / q;
        a_kl += 0.5f * (ratio * ratio + d * d - 1.f) - logf(ratio);
        a_ep += kHalfLog2PiPlusHalf + logf(p);
        a_eq += kHalfLog2PiPlusHalf + logf(q);
      }
    }
    a_kl = group_sum<G>(a_kl);
    a_ep = group_sum<G>(a_ep);
    a_eq = group_sum<G>(a_eq);
    if (rv && l == 0) {
      kl[r] = a_kl;
      if (ent_post) ent_post[r] = a_ep;
      if (ent_prior) ent_prior[r] = a_eq;
    }
  }
}

// loss_row = dyn_scale max(KL(sg(post) || prior), free) + rep_scale max(KL(post || sg(prior)), free)
//   d/dm1 = rep (m1-m2)/s2^2        d/ds1 = rep (s1/s2^2 - 1/s1)
//   d/dm2 = -dyn (m1-m2)/s2^2       d/ds2 = dyn (1/s2 - (s1^2 + (m1-m2)^2)/s2^3)
// gradient passes the clip where kl >= free, as in kl_bwd_kernel (catops.hip); `up` is the 1/(B T) of torch.mean.
// All four gradients are evaluated whichever outputs are requested (a dozen flops per element beside the loads).
__global__ __launch_bounds__(256) void gauss_kl_bwd_kernel(const float* __restrict__ m1, const float* __restrict__ s1,
                                                           const float* __restrict__ m2, const float* __restrict__ s2,
                                                           const float* __restrict__ kl, float* __restrict__ dm1,
                                                           float* __restrict__ ds1, float* __restrict__ dm2,
                                                           float* __restrict__ ds2, long R, int S, float free_nats,
                                                           float dyn_scale, float rep_scale, float up, int acc_post,
                                                           int acc_prior) {
  const long total = R * S;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const float pass = (kl[e / S] >= free_nats) ? up : 0.f;
    const float p = s1[e], q = s2[e], diff = m1[e] - m2[e];
    const float iq = 1.f / q, iq2 = iq * iq;
    const float rep = rep_scale * pass, dyn = dyn_scale * pass;
    const float gm1 = rep * diff * iq2;
    const float gs1 = rep * (p * iq2 - 1.f / p);
    const float gm2 = -dyn * diff * iq2;
    const float gs2 = dyn * (iq - (p * p + diff * diff) * iq2 * iq);
    if (dm1) dm1[e] = acc_post ? dm1[e] + gm1 : gm1;
    if (ds1) ds1[e] = acc_post ? ds1[e] + gs1 : gs1;
    if (dm2) dm2[e] = acc_prior ? dm2[e] + gm2 : gm2;
    if (ds2) ds2[e] = acc_prior ? ds2[e] + gs2 : gs2;
  }
}

static unsigned flat_blocks(long n, long cap) {
  long b = (n + 255) / 256;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}

constexpr int kMaxS = 1024;

}  // namespace dv3

using namespace dv3;

extern "C" int dv3_gauss_head_fwd(const float* raw, const float* eps, const unsigned long long* rng_state,
                                  unsigned long long rng_offset, float* eps_out, float* mean, float* std_out,
                                  float* stoch, long M, int S, int mean_act, int std_act, float min_std, int mode,
                                  const float* next_first, const float* init, float* next_out, void* stream) {
  if (M < 0 || S <= 0 || S > kMaxS || !raw || !stoch) return DV3_ERR_ARG;
  if (mean_act < kMeanNone || mean_act > kMeanTanh5 || std_act < kStdSoftplus || std_act > kStdIdentity)
    return DV3_ERR_ARG;
  if (!mode && !eps && !rng_state) return DV3_ERR_ARG;
  if ((next_first || init || next_out) && !(next_first && init && next_out)) return DV3_ERR_ARG;
  if (M == 0) return 0;
  hipLaunchKernelGGL(gauss_head_fwd_kernel, dim3(flat_blocks(M * S, 4096)), dim3(256), 0, (hipStream_t)stream, raw, eps,
                     rng_state, rng_offset, eps_out, mean, std_out, stoch, M, S, mean_act, std_act, min_std, mode,
                     next_first, init, next_out);
  return (int)hipGetLastError();
}

extern "C" int dv3_gauss_head_bwd(const float* dstoch, const float* dmean, const float* dstd, const float* raw,
                                  const float* eps, float* draw, long M, int S, int mean_act, int std_act, int mode,
                                  int accumulate, void* stream) {
  if (M < 0 || S <= 0 || S > kMaxS || !raw || !draw) return DV3_ERR_ARG;
  if (mean_act < kMeanNone || mean_act > kMeanTanh5 || std_act < kStdSoftplus || std_act > kStdIdentity)
    return DV3_ERR_ARG;
  if (!mode && dstoch && !eps) return DV3_ERR_ARG;
  if (M == 0) return 0;
  hipLaunchKernelGGL(gauss_head_bwd_kernel, dim3(flat_blocks(M * S, 4096)), dim3(256), 0, (hipStream_t)stream, dstoch,
                     dmean, dstd, raw, eps, draw, M, S, mean_act, std_act, mode, accumulate);
  return (int)hipGetLastError();
}

extern "C" int dv3_gauss_kl_fwd(const float* post_mean, const float* post_std, const float* prior_mean,
                                const float* prior_std, float* kl, float* ent_post, float* ent_prior, long R, int S,
                                void* stream) {
  if (R < 0 || S <= 0 || S > kMaxS || !post_mean || !post_std || !prior_mean || !prior_std || !kl) return DV3_ERR_ARG;
  if (R == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  int g = 4;
  while (g < 64 && g < S) g <<= 1;
#define DV3_GKL(G)                                                                                                    \
  hipLaunchKernelGGL((gauss_kl_fwd_kernel<G>), dim3(flat_blocks(R * G, 4096)), dim3(256), 0, s, post_mean, post_std, \
                     prior_mean, prior_std, kl, ent_post, ent_prior, R, S)
  switch (g) {
    case 4: DV3_GKL(4); break;
    case 8: DV3_GKL(8); break;
    case 16: DV3_GKL(16); break;
    case 32: DV3_GKL(32); break;
    default: DV3_GKL(64); break;
  }
#undef DV3_GKL
  return (int)hipGetLastError();
}

extern "C" int dv3_gauss_kl_bwd(const float* post_mean, const float* post_std, const float* prior_mean,
                                const float* prior_std, const float* kl, float* dpost_mean, float* dpost_std,
                                float* dprior_mean, float* dprior_std, long R, int S, float free_nats,
                                float dyn_scale, float rep_scale, float upstream, int acc_post, int acc_prior,
                                void* stream) {
  if (R < 0 || S <= 0 || S > kMaxS || !post_mean || !post_std || !prior_mean || !prior_std || !kl) return DV3_ERR_ARG;
  if (!dpost_mean && !dpost_std && !dprior_mean && !dprior_std) return DV3_ERR_ARG;
  if (R == 0) return 0;
  hipLaunchKernelGGL(gauss_kl_bwd_kernel, dim3(flat_blocks(R * S, 4096)), dim3(256), 0, (hipStream_t)stream, post_mean,
                     post_std, prior_mean, prior_std, kl, dpost_mean, dpost_std, dprior_mean, dprior_std, R, S,
                     free_nats, dyn_scale, rep_scale, upstream, acc_post, acc_prior);
  return (int)hipGetLastError();
}
