// Domain losses of DA Faster R-CNN (daod/modeling/meta_arch/da_faster_rcnn.py:228-272) on one-channel logit columns.
//
//   sfod_da_bce               BCE-with-logits against a constant label (image_dc_loss / instance_dc_loss), value and
//                             gradient in one launch + the fixed-order partial sum.
//   sfod_da_consistency_fwd   per ROI: p_img = mean over the P x P bins of ROIAlign(sigmoid(z_img)), p_ins = sigmoid(z_ins),
//                             loss = mean_live |p_img - p_ins|.
//   sfod_da_consistency_bwd   dz_ins per ROI; dz_img by an owner-per-pixel gather over the ROIs in a fixed order.
//
// The pooled map has ONE channel, so the lanes of a wavefront go on the ROI's pixel rows / columns and on its footprint
// pixels, not on channels.  The mean over all bins of a ROIAlign output is separable: with
//   Ay[y] = sum over the ROI's P * grid_h sample rows of the row's bilinear weight on pixel row y  / (count * P * P)
//   Ax[x] = sum over the ROI's P * grid_w sample columns of the column's bilinear weight on pixel column x
// (a sample row / column outside [-1, H] / [-1, W] dropped, as torchvision drops the sample), p_img = sum_y sum_x Ay[y] Ax[x]
// sigmoid(z_img[b, y, x]).  The forward keeps Ay | Ax per ROI ([R, H + W] fp32); the backward's gather reads them, so the
// adjoint is the transpose of exactly what the forward applied.  No float atomics anywhere: every sum has one owner and a
// fixed order, results are bit-identical from run to run.
#include "common.h"
#include <cmath>

#define DA_BLOCK 256
#define DA_WAVE 64

__device__ __forceinline__ float da_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// sum of v over the block's threads in a fixed (tree) order; every thread gets the result
template <int NT>
__device__ __forceinline__ float da_block_sum(float v, float* sm) {
  const int t = threadIdx.x;
  __syncthreads();
  sm[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s) sm[t] += sm[t + s];
    __syncthreads();
  }
  return sm[0];
}

// ---------------------------------------------------------------------------------------------
// BCE-with-logits against a constant label
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DA_BLOCK)
k_da_bce(const float* __restrict__ z, int64_t n, int ld, const float* __restrict__ rois, float label,
         const float* __restrict__ grad_scale, float* __restrict__ dz, float* __restrict__ ws) {
  __shared__ float sm[DA_BLOCK];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * DA_BLOCK + t;
  const bool live = i < n && (rois == nullptr || rois[i * 5] >= 0.f);
  float term = 0.f, zi = 0.f;
  if (live) {
    zi = z[i * ld];
    term = fmaxf(zi, 0.f) - zi * label + log1pf(expf(-fabsf(zi)));
  }
  const float bsum = da_block_sum<DA_BLOCK>(term, sm);
  const float bcnt = da_block_sum<DA_BLOCK>(live ? 1.f : 0.f, sm);      // <= 256: exact
  if (t == 0) { ws[2 * blockIdx.x] = bsum; ws[2 * blockIdx.x + 1] = bcnt; }
  if (grad_scale == nullptr) return;
  // the gradient needs the live count of ALL rows: every block counts the flags itself (integers: any order is exact)
  float n_live = (float)n;
  if (rois != nullptr) {
    int c = 0;
    for (int64_t j = t; j < n; j += DA_BLOCK) c += rois[j * 5] >= 0.f ? 1 : 0;
    n_live = da_block_sum<DA_BLOCK>((float)c, sm);      // < 2^24 rows (checked on the host): exact
  }
  if (i < n) dz[i * ld] = live ? (da_sigmoid(zi) - label) * (grad_scale[0] / fmaxf(n_live, 1.f)) : 0.f;
}

// out[0] = sum of the blocks' partial sums / max(live, 1), out[1] = live; partial [nblk][2], summed in a fixed order
__global__ void __launch_bounds__(DA_BLOCK)
k_da_sum_partials(const float* __restrict__ partial, int nblk, float* __restrict__ out) {
  __shared__ float sm[DA_BLOCK];
  const int t = threadIdx.x;
  float s = 0.f, c = 0.f;
  for (int i = t; i < nblk; i += DA_BLOCK) { s += partial[2 * i]; c += partial[2 * i + 1]; }
  s = da_block_sum<DA_BLOCK>(s, sm);
  c = da_block_sum<DA_BLOCK>(c, sm);
  if (t == 0) { out[0] = s / fmaxf(c, 1.f); out[1] = c; }
}

extern "C" int sfod_da_bce(const float* z, int64_t n, int ld, const float* rois, float label, float* loss,
                           const float* grad_scale, float* dz, float* ws, void* stream) {
  SFOD_REQUIRE(sfod_i64s_ok({n}) && sfod_ints_ok({ld}) && ld >= 1, "da_bce: negative or oversized extent");
  SFOD_REQUIRE(n < (1LL << 24) * DA_BLOCK && sfod_prod_fits({n, ld}, 1LL << 40), "da_bce: oversized problem");
  SFOD_REQUIRE(rois == nullptr || n < (1LL << 24), "da_bce: more masked rows than an exact fp32 count holds");
  SFOD_REQUIRE(std::isfinite(label), "da_bce: label must be finite");
  SFOD_REQUIRE(loss && ws && (n == 0 || z), "da_bce: null argument");
  SFOD_REQUIRE(grad_scale == nullptr || dz != nullptr, "da_bce: dz");
  hipStream_t s = (hipStream_t)stream;
  const int nblk = (int)((n + DA_BLOCK - 1) / DA_BLOCK);
  if (grad_scale && n > 0) (void)hipMemsetAsync(dz, 0, sizeof(float) * n * ld, s);      // the padding columns
  if (nblk > 0) {
    hipLaunchKernelGGL(k_da_bce, dim3(nblk), dim3(DA_BLOCK), 0, s, z, n, ld, rois, label, grad_scale, dz, ws);
    int rc = sfod_check_launch("da_bce");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_da_sum_partials, dim3(1), dim3(DA_BLOCK), 0, s, ws, nblk, loss);
  return sfod_check_launch("da_bce_sum");
}

// ---------------------------------------------------------------------------------------------
// consistency between the image-level and the instance-level probabilities
// ---------------------------------------------------------------------------------------------
// ROI geometry of csrc/roi_align.hip (roi_geom), per axis
struct DaAxis {
  float start, bin;
  int grid;
};

__device__ __forceinline__ DaAxis da_axis(float lo, float hi, float scale, int pooled, int sampling_ratio, int aligned) {
  DaAxis a;
  const float offset = aligned ? 0.5f : 0.f;
  a.start = lo * scale - offset;
  const float end = hi * scale - offset;
  float len = end - a.start;
  if (!aligned) len = fmaxf(len, 1.f);
  a.bin = len / (float)pooled;
  a.grid = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(len / (float)pooled);
  return a;
}

// weight of the axis' pooled * grid sample rows on pixel row `p` of an axis of n pixels (bilinear_setup of roi_align.hip,
// one axis of it)
__device__ __forceinline__ float da_axis_weight(const DaAxis a, int pooled, int n, int p) {
  float acc = 0.f;
  for (int ph = 0; ph < pooled; ++ph)
    for (int i = 0; i < a.grid; ++i) {
      float y = a.start + (float)ph * a.bin + ((float)i + .5f) * a.bin / (float)a.grid;
      if (y < -1.0f || y > (float)n) continue;
      if (y <= 0.f) y = 0.f;
      int lo = (int)y, hi;
      if (lo >= n - 1) { hi = lo = n - 1; y = (float)lo; } else hi = lo + 1;
      const float l = y - (float)lo, h = 1.f - l;
      if (lo == p) acc += h;
      if (hi == p) acc += l;
    }
  return acc;
}

// One wavefront per ROI.  Lanes on the pixel rows, then the pixel columns (Ay | Ax -> wts[r]), then on the map's pixels.
__global__ void __launch_bounds__(DA_WAVE)
k_da_consistency_fwd(const float* __restrict__ z_img, int B, int H, int W, int ld, const float* __restrict__ z_ins, int ld_ins,
                     const float* __restrict__ rois, int pooled, float scale, int sampling_ratio, int aligned,
                     float* __restrict__ p_img, float* __restrict__ sgn, float* __restrict__ term,
                     float* __restrict__ wts) {
  __shared__ float sm[DA_WAVE];
  const int r = blockIdx.x, t = threadIdx.x;
  const float* roi = rois + (int64_t)r * 5;
  float* wr = wts + (int64_t)r * (H + W);
  if (roi[0] < 0.f || roi[0] >= (float)B) {      // padding row (an image index past the batch is treated as one)
    for (int i = t; i < H + W; i += DA_WAVE) wr[i] = 0.f;
    if (t == 0) { p_img[r] = 0.f; sgn[r] = 0.f; term[r] = 0.f; }
    return;
  }
  const int b = (int)roi[0];
  const DaAxis ax = da_axis(roi[1], roi[3], scale, pooled, sampling_ratio, aligned);
  const DaAxis ay = da_axis(roi[2], roi[4], scale, pooled, sampling_ratio, aligned);
  const int c = ay.grid * ax.grid;
  const float inv = 1.f / ((float)(c > 1 ? c : 1) * (float)(pooled * pooled));
  for (int y = t; y < H; y += DA_WAVE) wr[y] = da_axis_weight(ay, pooled, H, y) * inv;
  for (int x = t; x < W; x += DA_WAVE) wr[H + x] = da_axis_weight(ax, pooled, W, x);
  __syncthreads();      // the block's own global writes are visible to it after the barrier
  const float* zb = z_img + (int64_t)b * H * W * ld;
  float acc = 0.f;
  for (int i = t; i < H * W; i += DA_WAVE) {
    const float w = wr[i / W] * wr[H + i % W];
    if (w != 0.f) acc += w * da_sigmoid(zb[(int64_t)i * ld]);
  }
  const float pi = da_block_sum<DA_WAVE>(acc, sm);
  if (t == 0) {
    const float d = pi - da_sigmoid(z_ins[(int64_t)r * ld_ins]);
    p_img[r] = pi;
    sgn[r] = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    term[r] = fabsf(d);
  }
}

// loss[0] = sum_r term[r] / max(n_live, 1), loss[1] = n_live; fixed order
__global__ void __launch_bounds__(DA_BLOCK)
k_da_consistency_sum(const float* __restrict__ term, const float* __restrict__ rois, int R, float* __restrict__ loss) {
  __shared__ float sm[DA_BLOCK];
  const int t = threadIdx.x;
  float s = 0.f, c = 0.f;
  for (int r = t; r < R; r += DA_BLOCK) {
    s += term[r];
    c += rois[(int64_t)r * 5] >= 0.f ? 1.f : 0.f;
  }
  s = da_block_sum<DA_BLOCK>(s, sm);
  c = da_block_sum<DA_BLOCK>(c, sm);
  if (t == 0) { loss[0] = s / fmaxf(c, 1.f); loss[1] = c; }
}

static int da_consistency_args(const char* what, int B, int H, int W, int ld, int ld_ins, int R, int pooled,
                               int sampling_ratio) {
  if (!sfod_ints_ok({B, H, W, ld, ld_ins, R, pooled, sampling_ratio}) || ld < 1 || ld_ins < 1 || H < 1 || W < 1 ||
      pooled < 1 || pooled > 16 || sampling_ratio > 16 || !sfod_prod_fits({B, H, W, ld}, 1LL << 40) ||
      !sfod_prod_fits({H, W}) || !sfod_prod_fits({R, (long long)H + W}, 1LL << 40) || !sfod_prod_fits({R, ld_ins}, 1LL << 40) ||
      R >= (1 << 24)) {
    sfod_set_error("bad argument: %s: negative or oversized extent (pooled in [1, 16], sampling_ratio in [0, 16])", what);
    return SFOD_EBADARG;
  }
  return 0;
}

extern "C" int sfod_da_consistency_fwd(const float* z_img, int B, int H, int W, int ld, const float* z_ins, int ld_ins,
                                       const float* rois, int R, int pooled, float scale, int sampling_ratio, int aligned,
                                       float* loss, float* p_img, float* sgn, float* term, float* wts, void* stream) {
  int rc = da_consistency_args("da_consistency_fwd", B, H, W, ld, ld_ins, R, pooled, sampling_ratio);
  if (rc) return rc;
  SFOD_REQUIRE(std::isfinite(scale) && scale > 0.f, "da_consistency_fwd: scale must be finite and > 0");
  SFOD_REQUIRE(loss && (R == 0 || (z_img && z_ins && rois && p_img && sgn && term && wts)), "da_consistency_fwd: null argument");
  hipStream_t s = (hipStream_t)stream;
  if (R > 0) {
    hipLaunchKernelGGL(k_da_consistency_fwd, dim3(R), dim3(DA_WAVE), 0, s, z_img, B, H, W, ld, z_ins, ld_ins, rois, pooled,
                       scale, sampling_ratio, aligned ? 1 : 0, p_img, sgn, term, wts);
    rc = sfod_check_launch("da_consistency_fwd");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_da_consistency_sum, dim3(1), dim3(DA_BLOCK), 0, s, term, rois, R, loss);
  return sfod_check_launch("da_consistency_sum");
}

// dz_ins[r] = -sgn_r * g / n_live * p_ins (1 - p_ins)
__global__ void __launch_bounds__(DA_BLOCK)
k_da_consistency_bwd_ins(const float* __restrict__ z_ins, int ld_ins, int R, const float* __restrict__ loss,
                         const float* __restrict__ sgn, const float* __restrict__ grad_scale,
                         float* __restrict__ dz_ins) {
  const int r = blockIdx.x * DA_BLOCK + threadIdx.x;
  if (r >= R) return;
  const float p = da_sigmoid(z_ins[(int64_t)r * ld_ins]);
  const float gn = grad_scale[0] / fmaxf(loss[1], 1.f);
  dz_ins[(int64_t)r * ld_ins] = -sgn[r] * gn * (p * (1.f - p));
}

// One owner per pixel and DA_PARTS lanes per owner: lane k walks the k-th contiguous part of the ROI rows in ROI order (the rows
// of its image only; a padding row has sgn 0 and zero weights), the owner adds the DA_PARTS partial sums in part order.  A fixed
// order, so the same bits every run; the walk is latency-bound (two dependent loads behind a branch), the parts run it in parallel.
#define DA_PARTS 16
#define DA_PIX (DA_BLOCK / DA_PARTS)
__global__ void __launch_bounds__(DA_BLOCK)
k_da_consistency_bwd_img(const float* __restrict__ z_img, int H, int W, int ld, const float* __restrict__ rois, int R,
                         const float* __restrict__ loss, const float* __restrict__ sgn, const float* __restrict__ wts,
                         const float* __restrict__ grad_scale, float* __restrict__ dz_img) {
  __shared__ float sm[DA_PARTS][DA_PIX];
  const int b = blockIdx.y;
  const int px = threadIdx.x % DA_PIX, part = threadIdx.x / DA_PIX;
  const int i = blockIdx.x * DA_PIX + px;
  const bool in = i < H * W;
  float acc = 0.f;
  if (in) {
    const int y = i / W, x = i % W;
    const int per = (R + DA_PARTS - 1) / DA_PARTS;
    const int r0 = part * per, r1 = min(R, r0 + per);
    for (int r = r0; r < r1; ++r) {
      if (rois[(int64_t)r * 5] != (float)b) continue;
      const float* wr = wts + (int64_t)r * (H + W);
      acc += sgn[r] * (wr[y] * wr[H + x]);
    }
  }
  sm[part][px] = acc;
  __syncthreads();
  if (!in || part != 0) return;
  float tot = sm[0][px];
#pragma unroll
  for (int k = 1; k < DA_PARTS; ++k) tot += sm[k][px];
  const int64_t o = ((int64_t)b * H * W + i) * ld;
  const float p = da_sigmoid(z_img[o]);
  dz_img[o] = tot * (grad_scale[0] / fmaxf(loss[1], 1.f)) * (p * (1.f - p));
}

extern "C" int sfod_da_consistency_bwd(const float* z_img, int B, int H, int W, int ld, const float* z_ins, int ld_ins,
                                       const float* rois, int R, const float* loss, const float* sgn, const float* wts,
                                       const float* grad_scale, float* dz_img, float* dz_ins, void* stream) {
  int rc = da_consistency_args("da_consistency_bwd", B, H, W, ld, ld_ins, R, 1, 0);
  if (rc) return rc;
  SFOD_REQUIRE(B <= 65535, "da_consistency_bwd: more images than a launch grid's second axis holds");
  SFOD_REQUIRE(loss && grad_scale && (B == 0 || (z_img && dz_img)) && (R == 0 || (z_ins && rois && sgn && wts && dz_ins)),
               "da_consistency_bwd: null argument");
  hipStream_t s = (hipStream_t)stream;
  if (R > 0) {
    (void)hipMemsetAsync(dz_ins, 0, sizeof(float) * (int64_t)R * ld_ins, s);      // the padding columns
    hipLaunchKernelGGL(k_da_consistency_bwd_ins, dim3((R + DA_BLOCK - 1) / DA_BLOCK), dim3(DA_BLOCK), 0, s, z_ins, ld_ins, R,
                       loss, sgn, grad_scale, dz_ins);
    rc = sfod_check_launch("da_consistency_bwd_ins");
    if (rc) return rc;
  }
  if (B > 0) {
    (void)hipMemsetAsync(dz_img, 0, sizeof(float) * (int64_t)B * H * W * ld, s);
    hipLaunchKernelGGL(k_da_consistency_bwd_img, dim3((H * W + DA_PIX - 1) / DA_PIX, B), dim3(DA_BLOCK), 0, s, z_img, H,
                       W, ld, rois, R, loss, sgn, wts, grad_scale, dz_img);
    rc = sfod_check_launch("da_consistency_bwd_img");
  }
  return rc;
}
