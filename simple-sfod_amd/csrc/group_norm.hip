// GroupNorm + ReLU of the box head's convolutions (MODEL.ROI_BOX_HEAD.NORM "GN"), forward and backward, on [R, PP, C] ROI
// tensors (NHWC; include/sfod_hip.h: sfod_group_norm_relu_fwd / _bwd).
//
// One workgroup of 256 threads works on one ROI at a time.  A thread owns ONE vector of V consecutive channels (V = 4 for
// an fp32 output, 8 for bf16 and operand pairs) and walks the ROI's pixels with stride TPR = 256 / (C / V); the first
// GN_CACHE / V pixels of its walk stay in registers, so that the hot shape (7 x 7 x 256: 50 KB per ROI) is read from
// memory once and a larger ROI re-reads only its tail (from L2: one ROI is at most a few hundred KB).  Sums over pixels are
// kept per thread and channel, laid into LDS as [TPR][C] and added per group by one thread in a fixed order: mean first,
// then the centred sum of squares.  Nothing here uses atomics: every result is a function of the inputs alone.
#include "common.h"
#include "conv_internal.h"

#define GN_THREADS 256
#define GN_CACHE 64          // floats of one tensor a thread keeps in registers
#define GN_MAX_C 1024        // LDS: [TPR][C] <= 256 * 8 floats per sum, one mean / rstd per group
#define GN_BWD_THREADS 512
#define GN_BWD_CACHE 32      // per tensor (y and dz)
#define GN_BWD_MAX_BLOCKS 1024

template <typename T, int V> __device__ __forceinline__ void gn_load(const T* p, float* out);
template <> __device__ __forceinline__ void gn_load<float, 4>(const float* p, float* out) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
}
template <> __device__ __forceinline__ void gn_load<float, 8>(const float* p, float* out) {
  gn_load<float, 4>(p, out);
  gn_load<float, 4>(p + 4, out + 4);
}
template <> __device__ __forceinline__ void gn_load<bf16_t, 8>(const bf16_t* p, float* out) {
  union { uint4 v; bf16_t h[8]; } u;
  u.v = *reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = (float)u.h[i];
}
template <typename T, int V> __device__ __forceinline__ void gn_store(T* p, const float* in);
template <> __device__ __forceinline__ void gn_store<float, 4>(float* p, const float* in) {
  *reinterpret_cast<float4*>(p) = make_float4(in[0], in[1], in[2], in[3]);
}
template <> __device__ __forceinline__ void gn_store<bf16_t, 8>(bf16_t* p, const float* in) {
  union { uint4 v; bf16_t h[8]; } u;
#pragma unroll
  for (int i = 0; i < 8; ++i) u.h[i] = (bf16_t)in[i];
  *reinterpret_cast<uint4*>(p) = u.v;
}
template <> __device__ __forceinline__ void gn_store<split_t, 8>(split_t* p, const float* in) { split_store8(p, in); }
template <> __device__ __forceinline__ void gn_store<splith_t, 8>(splith_t* p, const float* in) { split_store8(p, in); }

// the pre-activation of one element, in the order the header states (and the bound in DESIGN.md 4.7 counts): the forward
// and the backward's ReLU gate both call THIS, so the gate is the sign of the very value the forward activated
__device__ __forceinline__ float gn_xhat(float v, float mu, float rs) {
#pragma clang fp contract(off)
  return (v - mu) * rs;
}
__device__ __forceinline__ float gn_pre(float xh, float ga, float be) { return __builtin_fmaf(xh, ga, be); }

// sum of the [TPR][C] partials of group g (channels g * cpg ...), rows first: a fixed order
__device__ __forceinline__ float gn_group_sum(const float* red, int tpr, int C, int g, int cpg) {
  float s = 0.f;
  for (int t = 0; t < tpr; ++t)
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) s += red[t * C + c];
  return s;
}

template <typename TI, typename TO, int V, bool DUAL, int RELU>
__global__ void __launch_bounds__(GN_THREADS)
k_group_norm_relu_fwd(const TI* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ beta,
                      TO* __restrict__ z, split_t* __restrict__ z2, float* __restrict__ mean, float* __restrict__ rstd,
                      int R, int PP, int C, int groups, float eps) {
  constexpr int NC = GN_CACHE / V;
  __shared__ float red[GN_THREADS * 8];
  __shared__ float s_mean[GN_MAX_C], s_rstd[GN_MAX_C];
  const int CV = C / V, tpr = GN_THREADS / CV, cpg = C / groups;
  const int tid = threadIdx.x, tp = tid / CV, cv = tid - tp * CV;
  const bool active = tp < tpr;
  const int r = blockIdx.x;
  if (r >= R) return;
  const float n = (float)PP * (float)cpg;
  const TI* yr = y + (int64_t)r * PP * C + cv * V;
  int gi[V];
  float ga[V], be[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    gi[j] = active ? (cv * V + j) / cpg : 0;
    ga[j] = active ? gamma[cv * V + j] : 0.f;
    be[j] = active ? beta[cv * V + j] : 0.f;
  }
  float cache[NC][V];
  float acc[V];
  // ---- the mean ----
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int p = tp + k * tpr;
    if (active && p < PP) {
      gn_load<TI, V>(yr + (int64_t)p * C, cache[k]);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += cache[k][j];
    }
  }
  if (active)
    for (int p = tp + NC * tpr; p < PP; p += tpr) {
      float v[V];
      gn_load<TI, V>(yr + (int64_t)p * C, v);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += v[j];
    }
  if (active) {
#pragma unroll
    for (int j = 0; j < V; ++j) red[tp * C + cv * V + j] = acc[j];
  }
  __syncthreads();
  for (int g = tid; g < groups; g += GN_THREADS) s_mean[g] = gn_group_sum(red, tpr, C, g, cpg) / n;
  __syncthreads();
  // ---- the centred sum of squares ----
  float mu[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { mu[j] = s_mean[gi[j]]; acc[j] = 0.f; }
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int p = tp + k * tpr;
    if (active && p < PP) {
#pragma unroll
      for (int j = 0; j < V; ++j) { const float d = cache[k][j] - mu[j]; acc[j] = __builtin_fmaf(d, d, acc[j]); }
    }
  }
  if (active)
    for (int p = tp + NC * tpr; p < PP; p += tpr) {
      float v[V];
      gn_load<TI, V>(yr + (int64_t)p * C, v);
#pragma unroll
      for (int j = 0; j < V; ++j) { const float d = v[j] - mu[j]; acc[j] = __builtin_fmaf(d, d, acc[j]); }
    }
  if (active) {
#pragma unroll
    for (int j = 0; j < V; ++j) red[tp * C + cv * V + j] = acc[j];
  }
  __syncthreads();
  for (int g = tid; g < groups; g += GN_THREADS) {
    const float var = gn_group_sum(red, tpr, C, g, cpg) / n;
    const float rs = 1.0f / sqrtf(var + eps);
    s_rstd[g] = rs;
    mean[(int64_t)r * groups + g] = s_mean[g];
    rstd[(int64_t)r * groups + g] = rs;
  }
  __syncthreads();
  // ---- z = relu(xhat * gamma + beta), written as the next layer's operand ----
  if (!active) return;
  float rs[V];
#pragma unroll
  for (int j = 0; j < V; ++j) rs[j] = s_rstd[gi[j]];
  TO* zr = z + (int64_t)r * PP * C + cv * V;
  split_t* z2r = DUAL ? z2 + (int64_t)r * PP * C + cv * V : nullptr;
  auto emit = [&](int p, const float* v) {
    float o[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float zp = gn_pre(gn_xhat(v[j], mu[j], rs[j]), ga[j], be[j]);
      o[j] = RELU ? fmaxf(zp, 0.f) : zp;
    }
    gn_store<TO, V>(zr + (int64_t)p * C, o);
    if constexpr (DUAL) split_store8(z2r + (int64_t)p * C, o);
  };
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int p = tp + k * tpr;
    if (p < PP) emit(p, cache[k]);
  }
  for (int p = tp + NC * tpr; p < PP; p += tpr) {
    float v[V];
    gn_load<TI, V>(yr + (int64_t)p * C, v);
    emit(p, v);
  }
}

// Backward.  Two tensors are cached, so a workgroup has 512 threads with half the registers each (the hot ROI still fits:
// 512 x 32 floats per tensor).  A workgroup takes the ROIs blockIdx.x, blockIdx.x + gridDim.x, ... ; per ROI it forms, per channel,
// A_c = sum_p gz and B_c = sum_p gz * xhat (gz = dz gated by the recomputed pre-activation), from them the group means of
// g = gz * gamma and of g * xhat, and dy.  A_c / B_c also add up over the workgroup's ROIs (in ROI order) into its row of
// `ws` ([gridDim.x][2][C]: dbeta | dgamma partials), which k_group_norm_bwd_finish sums in row order.
template <typename T, typename TO, int V, int RELU>
__global__ void __launch_bounds__(GN_BWD_THREADS)
k_group_norm_relu_bwd(const T* __restrict__ dz, const T* __restrict__ y, const float* __restrict__ mean,
                      const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                      TO* __restrict__ dy, float* __restrict__ ws, int R, int PP, int C, int groups) {
  constexpr int NC = GN_BWD_CACHE / V;
  constexpr int CPT = GN_MAX_C / GN_BWD_THREADS;      // channels a thread totals
  __shared__ float redA[GN_BWD_THREADS * 8], redB[GN_BWD_THREADS * 8];
  __shared__ float chA[GN_MAX_C], chB[GN_MAX_C];
  __shared__ float s_m1[GN_MAX_C], s_m2[GN_MAX_C];
  const int CV = C / V, tpr = GN_BWD_THREADS / CV, cpg = C / groups;
  const int tid = threadIdx.x, tp = tid / CV, cv = tid - tp * CV;
  const bool active = tp < tpr;
  const float n = (float)PP * (float)cpg;
  int gi[V];
  float ga[V], be[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    gi[j] = active ? (cv * V + j) / cpg : 0;
    ga[j] = active ? gamma[cv * V + j] : 0.f;
    be[j] = active ? beta[cv * V + j] : 0.f;
  }
  float totA[CPT], totB[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) totA[i] = totB[i] = 0.f;
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const T* yr = y + (int64_t)r * PP * C + cv * V;
    const T* dzr = dz + (int64_t)r * PP * C + cv * V;
    float mu[V], rs[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      mu[j] = mean[(int64_t)r * groups + gi[j]];
      rs[j] = rstd[(int64_t)r * groups + gi[j]];
    }
    float cy[NC][V], cg[NC][V];      // xhat and the gated dz of the cached pixels
    float a[V], b[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = b[j] = 0.f;
    auto gate = [&](float* v, float* g) {      // v: y -> xhat, g: dz -> gz; sums
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float xh = gn_xhat(v[j], mu[j], rs[j]);
        const float gz = (!RELU || gn_pre(xh, ga[j], be[j]) > 0.f) ? g[j] : 0.f;
        v[j] = xh;
        g[j] = gz;
        a[j] += gz;
        b[j] = __builtin_fmaf(gz, xh, b[j]);
      }
    };
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int p = tp + k * tpr;
      if (active && p < PP) {
        gn_load<T, V>(yr + (int64_t)p * C, cy[k]);
        gn_load<T, V>(dzr + (int64_t)p * C, cg[k]);
        gate(cy[k], cg[k]);
      }
    }
    if (active)
      for (int p = tp + NC * tpr; p < PP; p += tpr) {
        float v[V], g[V];
        gn_load<T, V>(yr + (int64_t)p * C, v);
        gn_load<T, V>(dzr + (int64_t)p * C, g);
        gate(v, g);
      }
    if (active) {
#pragma unroll
      for (int j = 0; j < V; ++j) { redA[tp * C + cv * V + j] = a[j]; redB[tp * C + cv * V + j] = b[j]; }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int c = tid + i * GN_BWD_THREADS;
      if (c < C) {
        float sa = 0.f, sb = 0.f;
        for (int t = 0; t < tpr; ++t) { sa += redA[t * C + c]; sb += redB[t * C + c]; }
        totA[i] += sa;
        totB[i] += sb;
        const float gc = gamma[c];
        chA[c] = sa * gc;
        chB[c] = sb * gc;
      }
    }
    __syncthreads();
    for (int g = tid; g < groups; g += GN_BWD_THREADS) {
      float s1 = 0.f, s2 = 0.f;
      for (int c = g * cpg; c < (g + 1) * cpg; ++c) { s1 += chA[c]; s2 += chB[c]; }
      s_m1[g] = s1 / n;
      s_m2[g] = s2 / n;
    }
    __syncthreads();
    if (active) {
      float m1[V], m2[V];
#pragma unroll
      for (int j = 0; j < V; ++j) { m1[j] = s_m1[gi[j]]; m2[j] = s_m2[gi[j]]; }
      TO* dyr = dy + (int64_t)r * PP * C + cv * V;
      auto emit = [&](int p, const float* xh, const float* gz) {
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = rs[j] * __builtin_fmaf(-xh[j], m2[j], gz[j] * ga[j] - m1[j]);
        gn_store<TO, V>(dyr + (int64_t)p * C, o);
      };
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int p = tp + k * tpr;
        if (p < PP) emit(p, cy[k], cg[k]);
      }
      for (int p = tp + NC * tpr; p < PP; p += tpr) {
        float v[V], g[V];
        gn_load<T, V>(yr + (int64_t)p * C, v);
        gn_load<T, V>(dzr + (int64_t)p * C, g);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float xh = gn_xhat(v[j], mu[j], rs[j]);
          g[j] = (!RELU || gn_pre(xh, ga[j], be[j]) > 0.f) ? g[j] : 0.f;
          v[j] = xh;
        }
        emit(p, v, g);
      }
    }
    // (the next ROI's first write to redA / redB comes after this ROI's last read of them: the two barriers above)
  }
  float* row = ws + (int64_t)blockIdx.x * 2 * C;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = tid + i * GN_BWD_THREADS;
    if (c < C) { row[c] = totA[i]; row[C + c] = totB[i]; }
  }
}

// dbeta[c] (+)= sum_rows ws[row][c], dgamma[c] (+)= sum_rows ws[row][C + c]: 16 columns x 16 row slices per workgroup, each
// slice summed in row order in fp64, the slices in slice order
__global__ void __launch_bounds__(256)
k_group_norm_bwd_finish(const float* __restrict__ ws, int rows, int C, float* __restrict__ dgamma,
                        float* __restrict__ dbeta, int accumulate) {
  __shared__ double part[16][16];
  const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + cl;      // of 2 * C
  double s = 0.0;
  if (col < 2 * C)
    for (int r = sl; r < rows; r += 16) s += (double)ws[(int64_t)r * 2 * C + col];
  part[sl][cl] = s;
  __syncthreads();
  if (sl == 0 && col < 2 * C) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += part[i][cl];
    float* out = col < C ? dbeta + col : dgamma + (col - C);
    *out = accumulate ? *out + (float)t : (float)t;
  }
}

static int gn_check(int R, int PP, int C, int groups, int V) {
  SFOD_REQUIRE_EXTENTS("group_norm", R, PP, C, groups);
  SFOD_REQUIRE(PP >= 1 && C >= 1 && groups >= 1, "group_norm: PP, C and groups must be positive");
  SFOD_REQUIRE(C <= GN_MAX_C, "group_norm: C above 1024");
  SFOD_REQUIRE(C % groups == 0, "group_norm: C not a multiple of groups");
  SFOD_REQUIRE(C % V == 0, "group_norm: C not a multiple of the vector width (8 for bf16 and operand pairs, 4 for fp32)");
  SFOD_REQUIRE(sfod_prod_fits({R, PP, C}, 1LL << 40) && sfod_prod_fits({PP, C}) && sfod_prod_fits({R, groups}),
               "group_norm: oversized tensor");
  return 0;
}

extern "C" int sfod_group_norm_relu_fwd(const void* y, const float* gamma, const float* beta, void* z, void* z_grad_operand,
                                        float* mean, float* rstd, int R, int PP, int C, int groups, float eps, int relu,
                                        int y_dt, int z_dt, void* stream) {
  SFOD_REQUIRE(y_dt == SFOD_F32 || y_dt == SFOD_BF16, "group_norm_relu_fwd: y is fp32 or bf16 (convolutions on operand pairs write fp32)");
  SFOD_REQUIRE(z_dt == y_dt || (y_dt == SFOD_F32 && sfod_is_pairs(z_dt)),
               "group_norm_relu_fwd: z has y's type, or operand pairs from an fp32 y");
  SFOD_REQUIRE(z_grad_operand == nullptr || z_dt == SFOD_F16X3,
               "group_norm_relu_fwd: the second (bf16-pair) output accompanies SFOD_F16X3 pairs");
  SFOD_REQUIRE(relu == 0 || relu == 1, "group_norm_relu_fwd: relu is 0 or 1");
  SFOD_REQUIRE(eps >= 0.f && eps < 1e30f, "group_norm_relu_fwd: eps must be finite and >= 0");
  const int V = z_dt == SFOD_F32 ? 4 : 8;
  const int rc = gn_check(R, PP, C, groups, V);
  if (rc) return rc;
  if (R == 0) return 0;      // (an empty tensor has no address)
  SFOD_REQUIRE(y && gamma && beta && z && mean && rstd, "group_norm_relu_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(TI, TO, VV, DUAL, RL)                                                                                   \
  hipLaunchKernelGGL((k_group_norm_relu_fwd<TI, TO, VV, DUAL, RL>), dim3(R), dim3(GN_THREADS), 0, s, (const TI*)y, gamma, \
                     beta, (TO*)z, (split_t*)z_grad_operand, mean, rstd, R, PP, C, groups, eps)
#define LAUNCH2(TI, TO, VV, DUAL) do { if (relu) LAUNCH(TI, TO, VV, DUAL, 1); else LAUNCH(TI, TO, VV, DUAL, 0); } while (0)
  if (z_grad_operand != nullptr) LAUNCH2(float, splith_t, 8, true);
  else if (z_dt == SFOD_F16X3) LAUNCH2(float, splith_t, 8, false);
  else if (z_dt == SFOD_BF16X3) LAUNCH2(float, split_t, 8, false);
  else if (z_dt == SFOD_F32) LAUNCH2(float, float, 4, false);
  else LAUNCH2(bf16_t, bf16_t, 8, false);
#undef LAUNCH2
#undef LAUNCH
  return sfod_check_launch("group_norm_relu_fwd");
}

static int gn_bwd_blocks(int R) { return R < GN_BWD_MAX_BLOCKS ? R : GN_BWD_MAX_BLOCKS; }

extern "C" int64_t sfod_group_norm_bwd_ws_floats(int R, int C) {
  SFOD_REQUIRE_EXTENTS("group_norm_bwd_ws_floats", R, C);
  SFOD_REQUIRE(C <= GN_MAX_C, "group_norm: C above 1024");
  return (int64_t)(gn_bwd_blocks(R) > 0 ? gn_bwd_blocks(R) : 1) * 2 * C;
}

extern "C" int sfod_group_norm_relu_bwd(const void* dz, const void* y, const float* mean, const float* rstd,
                                        const float* gamma, const float* beta, void* dy, float* dgamma, float* dbeta,
                                        float* ws, int R, int PP, int C, int groups, int relu, int accumulate, int dt,
                                        int dy_dt, void* stream) {
  SFOD_REQUIRE(dt == SFOD_F32 || dt == SFOD_BF16, "group_norm_relu_bwd: dz and y are fp32 or bf16");
  SFOD_REQUIRE(dy_dt == dt || (dt == SFOD_F32 && dy_dt == SFOD_BF16X3),
               "group_norm_relu_bwd: dy has dz's type, or bf16 pairs from fp32 (the operand of the backward products)");
  SFOD_REQUIRE(relu == 0 || relu == 1, "group_norm_relu_bwd: relu is 0 or 1");
  SFOD_REQUIRE(accumulate == 0 || accumulate == 1, "group_norm_relu_bwd: accumulate is 0 or 1");
  const int V = dy_dt == SFOD_F32 ? 4 : 8;
  const int rc = gn_check(R, PP, C, groups, V);
  if (rc) return rc;
  SFOD_REQUIRE(dgamma && dbeta, "group_norm_relu_bwd: null pointer");
  SFOD_REQUIRE(R == 0 || (dz && y && mean && rstd && gamma && beta && dy && ws), "group_norm_relu_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (R == 0) {      // no ROI (empty tensors have no address): the parameter gradients of this call are zero
    if (!accumulate) {
      hipMemsetAsync(dgamma, 0, sizeof(float) * C, s);
      hipMemsetAsync(dbeta, 0, sizeof(float) * C, s);
    }
    return sfod_check_launch("group_norm_relu_bwd");
  }
  const int nb = gn_bwd_blocks(R);
#define LAUNCH(T, TO, VV, RL)                                                                                       \
  hipLaunchKernelGGL((k_group_norm_relu_bwd<T, TO, VV, RL>), dim3(nb), dim3(GN_BWD_THREADS), 0, s, (const T*)dz, (const T*)y, \
                     mean, rstd, gamma, beta, (TO*)dy, ws, R, PP, C, groups)
#define LAUNCH2(T, TO, VV) do { if (relu) LAUNCH(T, TO, VV, 1); else LAUNCH(T, TO, VV, 0); } while (0)
  if (dy_dt == SFOD_BF16X3) LAUNCH2(float, split_t, 8);
  else if (dt == SFOD_F32) LAUNCH2(float, float, 4);
  else LAUNCH2(bf16_t, bf16_t, 8);
#undef LAUNCH2
#undef LAUNCH
  hipLaunchKernelGGL(k_group_norm_bwd_finish, dim3(cdiv(2 * C, 16)), dim3(256), 0, s, ws, nb, C, dgamma, dbeta, accumulate);
  return sfod_check_launch("group_norm_relu_bwd");
}

SFOD_DEFINE_F16_POLL(sfod_f16_poll_gn)
