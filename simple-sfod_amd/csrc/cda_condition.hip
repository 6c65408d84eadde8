// Class conditioning of the instance-level domain classifier of conditional DA Faster R-CNN
// (daod/modeling/meta_arch/cda_faster_rcnn.py:22-33, 263-283): the classifier reads the outer product of the box features and
// the detached class probabilities, and can weight each ROI by the entropy of its prediction.
//
//   sfod_cda_condition_fwd    p = softmax(scores), w = 1 + exp(-H(p)), x[r, c * D + d] = p[r, c] * f[r, d], written as the
//                             operand of the GEMM that follows (fp32, bf16, bf16 pairs, half pairs; for half pairs also the
//                             bf16 pairs the weight gradient reads, from the same registers).
//   sfod_cda_condition_bwd    df[r, d] = sum_c p[r, c] * dx[r, c * D + d], c ascending, one owner per element, summed in double.
//   sfod_da_bce_weighted      sfod_da_bce (csrc/da_losses.hip, left as it is) with a weight per row.
//
// Forward: one workgroup per ROI row.  The first wavefront forms p (and w) of the row, in double, into LDS.  The row's
// C * D / 8 vectors of 8 elements go over the threads as (class group, vector of f): a thread keeps its 8 values of f in
// registers and walks the classes of its group, so that the stores of one class are consecutive 32-byte (fp32, pairs) or
// 16-byte (bf16) pieces over consecutive lanes.  The kernel is store-bound: C * D elements written per D read.
// No float atomics anywhere: every sum has one owner and a fixed order.
#include "common.h"
#include "conv_internal.h"
#include <cmath>

#define CDA_BLOCK 256
#define CDA_WAVE 64
#define CDA_ENTROPY_EPS 1e-5f      // daod/modeling/utils.py entropy(): -sum p log(p + 1e-5)

template <typename T> __device__ __forceinline__ void cda_load8(const T* p, float* out);
template <> __device__ __forceinline__ void cda_load8<float>(const float* p, float* out) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
  out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
}
template <> __device__ __forceinline__ void cda_load8<bf16_t>(const bf16_t* p, float* out) {
  union { uint4 v; bf16_t h[8]; } u;
  u.v = *reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = (float)u.h[i];
}
template <> __device__ __forceinline__ void cda_load8<split_t>(const split_t* p, float* out) { split_load8(p, out); }
template <> __device__ __forceinline__ void cda_load8<splith_t>(const splith_t* p, float* out) { split_load8(p, out); }

template <typename T> __device__ __forceinline__ void cda_store8(T* p, const float* in);
template <> __device__ __forceinline__ void cda_store8<float>(float* p, const float* in) {
  store16<false>(p, make_uint4(__float_as_uint(in[0]), __float_as_uint(in[1]), __float_as_uint(in[2]), __float_as_uint(in[3])));
  store16<false>(p + 4, make_uint4(__float_as_uint(in[4]), __float_as_uint(in[5]), __float_as_uint(in[6]), __float_as_uint(in[7])));
}
template <> __device__ __forceinline__ void cda_store8<bf16_t>(bf16_t* p, const float* in) {
  union { uint4 v; bf16_t h[8]; } u;
#pragma unroll
  for (int i = 0; i < 8; ++i) u.h[i] = (bf16_t)in[i];
  store16<false>(p, u.v);
}
template <> __device__ __forceinline__ void cda_store8<split_t>(split_t* p, const float* in) { split_store8<false>(p, in); }
template <> __device__ __forceinline__ void cda_store8<splith_t>(splith_t* p, const float* in) { split_store8<false>(p, in); }

__device__ __forceinline__ double cda_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// p and w of one row, by one wavefront (lanes on the classes, stride 64).  The row's C scalars are formed in double: they cost
// nothing beside the C * D stores, and with them x is the storage type's rounding of the exact product p * f (to double's
// precision) -- a 16-bit output cannot flip a rounding on the last bit of an fp32 softmax.  ps: the row's p in LDS, for the
// products; pr / wr: their fp32 roundings, kept for the backward and the loss.  Sums go through the wavefront's butterfly: a
// fixed order.
__device__ __forceinline__ void cda_row_probs(const float* __restrict__ sc, int C, int entropy, double* ps, float* __restrict__ pr,
                                              float* __restrict__ wr) {
  const int lane = threadIdx.x;
  float mf = -INFINITY;
  for (int c = lane; c < C; c += CDA_WAVE) mf = fmaxf(mf, sc[c]);
  const double m = (double)wave_max(mf);
  double s = 0.0;
  for (int c = lane; c < C; c += CDA_WAVE) s += exp((double)sc[c] - m);
  s = cda_wave_sum(s);
  double h = 0.0;
  for (int c = lane; c < C; c += CDA_WAVE) {
    const double p = exp((double)sc[c] - m) / s;
    ps[c] = p;
    pr[c] = (float)p;
    h += p * log(p + (double)CDA_ENTROPY_EPS);
  }
  if (entropy) {
    h = cda_wave_sum(h);
    if (lane == 0) *wr = (float)(1.0 + exp(h));      // h = -H
  } else if (lane == 0) {
    *wr = 1.f;
  }
}

template <typename TI, typename TO, bool DUAL>
__global__ void __launch_bounds__(CDA_BLOCK)
k_cda_condition_fwd(const TI* __restrict__ f, const float* __restrict__ scores, int ld, const float* __restrict__ rois, int D,
                    int C, int entropy, TO* __restrict__ x, split_t* __restrict__ x2, float* __restrict__ p,
                    float* __restrict__ w) {
  extern __shared__ double ps[];      // [C]
  const int r = blockIdx.x, t = threadIdx.x;
  const int DV = D >> 3;
  const bool live = rois[(int64_t)r * 5] >= 0.f;
  float* pr = p + (int64_t)r * C;
  if (live) {
    if (t < CDA_WAVE) cda_row_probs(scores + (int64_t)r * ld, C, entropy, ps, pr, w + r);
  } else {      // a padding row: zeros, whatever its score row holds
    for (int c = t; c < C; c += CDA_BLOCK) pr[c] = 0.f;
    if (t == 0) w[r] = 0.f;
  }
  __syncthreads();
  const int lanes = DV < CDA_BLOCK ? DV : CDA_BLOCK;      // threads along f's vectors
  const int G = CDA_BLOCK / lanes;                        // class groups
  const int cg = t / lanes, tv = t - cg * lanes;
  if (cg >= G) return;
  const TI* fr = f + (int64_t)r * D;
  TO* xr = x + (int64_t)r * C * D;
  split_t* x2r = DUAL ? x2 + (int64_t)r * C * D : nullptr;
  for (int dv = tv; dv < DV; dv += lanes) {
    double fv[8];
    if (live) {
      float ff[8];
      cda_load8<TI>(fr + dv * 8, ff);
#pragma unroll
      for (int j = 0; j < 8; ++j) fv[j] = (double)ff[j];
    }
    for (int c = cg; c < C; c += G) {
      float o[8];
      if (live) {
        const double pc = ps[c];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (float)(pc * fv[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = 0.f;
      }
      const int64_t off = (int64_t)c * D + dv * 8;
      cda_store8<TO>(xr + off, o);
      if constexpr (DUAL) split_store8<false>(x2r + off, o);
    }
  }
}

#define CDA_MAX_C 4096      // the row's probabilities in LDS as doubles: 32 KB

static int cda_check(const char* what, int R, int D, int C) {
  if (!sfod_ints_ok({R, D, C}) || D < 8 || D % 8 != 0 || C < 2 || C > CDA_MAX_C || !sfod_prod_fits({C, D}) ||
      !sfod_prod_fits({R, C, D}, 1LL << 40)) {
    sfod_set_error("bad argument: %s: needs R >= 0, D a positive multiple of 8, 4096 >= C >= 2 and R * C * D < 2^40", what);
    return SFOD_EBADARG;
  }
  return 0;
}

static bool cda_dt_ok(int dt) { return dt == SFOD_F32 || dt == SFOD_BF16 || dt == SFOD_BF16X3 || dt == SFOD_F16X3; }

extern "C" int sfod_cda_condition_fwd(const void* f, int f_dt, const float* scores, int ld, const float* rois, int R, int D,
                                      int C, int entropy, void* x, int x_dt, void* x_grad_operand, float* p, float* w,
                                      void* stream) {
  int rc = cda_check("cda_condition_fwd", R, D, C);
  if (rc) return rc;
  SFOD_REQUIRE(cda_dt_ok(f_dt) && cda_dt_ok(x_dt), "cda_condition_fwd: storage types are SFOD_F32 / BF16 / BF16X3 / F16X3");
  SFOD_REQUIRE(sfod_ints_ok({ld}) && ld >= C && sfod_prod_fits({R, ld}, 1LL << 40), "cda_condition_fwd: ld below C or oversized");
  SFOD_REQUIRE(entropy == 0 || entropy == 1, "cda_condition_fwd: entropy is 0 or 1");
  SFOD_REQUIRE(x_grad_operand == nullptr || x_dt == SFOD_F16X3,
               "cda_condition_fwd: the second (bf16-pair) output accompanies SFOD_F16X3 pairs");
  if (R == 0) return 0;      // (an empty tensor has no address)
  SFOD_REQUIRE(f && scores && rois && x && p && w, "cda_condition_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(TI, TO, DUAL)                                                                                              \
  hipLaunchKernelGGL((k_cda_condition_fwd<TI, TO, DUAL>), dim3(R), dim3(CDA_BLOCK), sizeof(double) * C, s, (const TI*)f, scores, \
                     ld, rois, D, C, entropy, (TO*)x, (split_t*)x_grad_operand, p, w)
#define LAUNCH_OUT(TI)                                                      \
  do {                                                                      \
    if (x_grad_operand != nullptr) LAUNCH(TI, splith_t, true);              \
    else if (x_dt == SFOD_F16X3) LAUNCH(TI, splith_t, false);               \
    else if (x_dt == SFOD_BF16X3) LAUNCH(TI, split_t, false);               \
    else if (x_dt == SFOD_BF16) LAUNCH(TI, bf16_t, false);                  \
    else LAUNCH(TI, float, false);                                          \
  } while (0)
  if (f_dt == SFOD_F32) LAUNCH_OUT(float);
  else if (f_dt == SFOD_BF16) LAUNCH_OUT(bf16_t);
  else if (f_dt == SFOD_BF16X3) LAUNCH_OUT(split_t);
  else LAUNCH_OUT(splith_t);
#undef LAUNCH_OUT
#undef LAUNCH
  return sfod_check_launch("cda_condition_fwd");
}

// One thread owns V consecutive elements of df (16 bytes) and adds the row's C terms in class order, in double (free beside
// the C * D loads): df is the rounding to fp32, then to its storage type, of the exact sum -- like the forward's x, a bf16 df
// does not hang on the last bit of an fp32 accumulation.
template <typename T, int V>
__global__ void __launch_bounds__(CDA_BLOCK)
k_cda_condition_bwd(const T* __restrict__ dx, const float* __restrict__ p, const float* __restrict__ rois, int D, int C,
                    T* __restrict__ df, int R) {
  const int dv = blockIdx.x * CDA_BLOCK + threadIdx.x;
  if (dv >= D / V) return;
  for (int r = blockIdx.y; r < R; r += gridDim.y) {
    double acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.0;
    if (rois[(int64_t)r * 5] >= 0.f) {
      const T* dxr = dx + (int64_t)r * C * D + dv * V;
      const float* pr = p + (int64_t)r * C;
      for (int c = 0; c < C; ++c) {
        const double pc = (double)pr[c];
        float v[V];
        if constexpr (V == 4) {
          const float4 a = *reinterpret_cast<const float4*>(dxr + (int64_t)c * D);
          v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        } else {
          cda_load8<T>(dxr + (int64_t)c * D, v);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = __builtin_fma(pc, (double)v[j], acc[j]);
      }
    }
    T* o = df + (int64_t)r * D + dv * V;
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(o) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
    } else {
      union { uint4 v; bf16_t h[8]; } u;
#pragma unroll
      for (int j = 0; j < V; ++j) u.h[j] = (bf16_t)(float)acc[j];
      *reinterpret_cast<uint4*>(o) = u.v;
    }
  }
}

extern "C" int sfod_cda_condition_bwd(const void* dx, int dt, const float* p, const float* rois, int R, int D, int C, void* df,
                                      void* stream) {
  int rc = cda_check("cda_condition_bwd", R, D, C);
  if (rc) return rc;
  SFOD_REQUIRE(dt == SFOD_F32 || dt == SFOD_BF16, "cda_condition_bwd: dx and df are fp32 or bf16 (what the data-gradient GEMM writes)");
  if (R == 0) return 0;
  SFOD_REQUIRE(dx && p && rois && df, "cda_condition_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int gy = R < 65535 ? R : 65535;      // (rows beyond a grid's second axis: a workgroup walks them)
  if (dt == SFOD_F32)
    hipLaunchKernelGGL((k_cda_condition_bwd<float, 4>), dim3(cdiv(D / 4, CDA_BLOCK), gy), dim3(CDA_BLOCK), 0, s, (const float*)dx,
                       p, rois, D, C, (float*)df, R);
  else
    hipLaunchKernelGGL((k_cda_condition_bwd<bf16_t, 8>), dim3(cdiv(D / 8, CDA_BLOCK), gy), dim3(CDA_BLOCK), 0, s,
                       (const bf16_t*)dx, p, rois, D, C, (bf16_t*)df, R);
  return sfod_check_launch("cda_condition_bwd");
}

// ---------------------------------------------------------------------------------------------
// BCE-with-logits against a constant label, a weight per row
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float cda_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// sum of v over the block's threads in a fixed (tree) order; every thread gets the result (da_block_sum of da_losses.hip)
__device__ __forceinline__ float cda_block_sum(float v, float* sm) {
  const int t = threadIdx.x;
  __syncthreads();
  sm[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = CDA_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) sm[t] += sm[t + s];
    __syncthreads();
  }
  return sm[0];
}

// ws: [nblk][2] partials (sum of w * term, live count), then one float: the sum of the live weights.  Every block forms that
// sum itself, over ALL rows in the same order (a strided walk, then the tree), so that the gradient's divisor has the same
// bits in every block and is the loss's divisor.
__global__ void __launch_bounds__(CDA_BLOCK)
k_da_bce_weighted(const float* __restrict__ z, int64_t n, int ld, const float* __restrict__ rois,
                  const float* __restrict__ weight, float label, const float* __restrict__ grad_scale,
                  float* __restrict__ dz, float* __restrict__ ws, int nblk) {
  __shared__ float sm[CDA_BLOCK];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * CDA_BLOCK + t;
  const bool live = i < n && (rois == nullptr || rois[i * 5] >= 0.f);
  float term = 0.f, zi = 0.f, wi = 0.f;
  if (live) {
    zi = z[i * ld];
    wi = weight[i];
    term = wi * (fmaxf(zi, 0.f) - zi * label + log1pf(expf(-fabsf(zi))));
  }
  const float bsum = cda_block_sum(term, sm);
  const float bcnt = cda_block_sum(live ? 1.f : 0.f, sm);      // <= 256: exact
  if (t == 0) { ws[2 * blockIdx.x] = bsum; ws[2 * blockIdx.x + 1] = bcnt; }
  float wl = 0.f;
  for (int64_t j = t; j < n; j += CDA_BLOCK)
    if (rois == nullptr || rois[j * 5] >= 0.f) wl += weight[j];
  const float wsum = cda_block_sum(wl, sm);
  if (blockIdx.x == 0 && t == 0) ws[2 * nblk] = wsum;
  if (grad_scale == nullptr) return;
  if (i < n) dz[i * ld] = (live && wsum > 0.f) ? (cda_sigmoid(zi) - label) * (grad_scale[0] * (wi / wsum)) : 0.f;
}

// out[0] = sum of the blocks' partial sums / the sum of the live weights (0 without a live row), out[1] = live
__global__ void __launch_bounds__(CDA_BLOCK)
k_da_bce_weighted_sum(const float* __restrict__ ws, int nblk, float* __restrict__ out) {
  __shared__ float sm[CDA_BLOCK];
  const int t = threadIdx.x;
  float s = 0.f, c = 0.f;
  for (int i = t; i < nblk; i += CDA_BLOCK) { s += ws[2 * i]; c += ws[2 * i + 1]; }
  s = cda_block_sum(s, sm);
  c = cda_block_sum(c, sm);
  if (t == 0) {
    const float wsum = nblk > 0 ? ws[2 * nblk] : 0.f;
    out[0] = (c > 0.f && wsum > 0.f) ? s / wsum : 0.f;
    out[1] = c;
  }
}

extern "C" int64_t sfod_da_bce_weighted_ws_floats(int64_t n) {
  if (n < 0 || n > (1LL << 40)) return SFOD_EBADARG;
  return 2 * ((n + CDA_BLOCK - 1) / CDA_BLOCK) + 1;
}

extern "C" int sfod_da_bce_weighted(const float* z, int64_t n, int ld, const float* rois, const float* weight, float label,
                                    float* loss, const float* grad_scale, float* dz, float* ws, void* stream) {
  SFOD_REQUIRE(sfod_i64s_ok({n}) && sfod_ints_ok({ld}) && ld >= 1, "da_bce_weighted: negative or oversized extent");
  SFOD_REQUIRE(n < (1LL << 24) && sfod_prod_fits({n, ld}, 1LL << 40), "da_bce_weighted: more rows than an exact fp32 count holds");
  SFOD_REQUIRE(std::isfinite(label), "da_bce_weighted: label must be finite");
  SFOD_REQUIRE(loss && ws && (n == 0 || (z && weight)), "da_bce_weighted: null argument");
  SFOD_REQUIRE(grad_scale == nullptr || dz != nullptr, "da_bce_weighted: dz");
  hipStream_t s = (hipStream_t)stream;
  const int nblk = (int)((n + CDA_BLOCK - 1) / CDA_BLOCK);
  if (grad_scale && n > 0) (void)hipMemsetAsync(dz, 0, sizeof(float) * n * ld, s);      // the padding columns
  if (nblk > 0) {
    hipLaunchKernelGGL(k_da_bce_weighted, dim3(nblk), dim3(CDA_BLOCK), 0, s, z, n, ld, rois, weight, label, grad_scale, dz, ws,
                       nblk);
    int rc = sfod_check_launch("da_bce_weighted");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_da_bce_weighted_sum, dim3(1), dim3(CDA_BLOCK), 0, s, ws, nblk, loss);
  return sfod_check_launch("da_bce_weighted_sum");
}

SFOD_DEFINE_F16_POLL(sfod_f16_poll_cda)
