// COCOeval's per-image matching (pycocotools cocoeval.py computeIoU + evaluateImg, as restated by
// evaluation.py::COCOevalBBox.evaluate / _evaluate_img, which is the definition) for a batch of images in one launch.
//
// One wavefront per image.  The loop over detections is serial (a detection sees the ground truths the better-scored ones
// of its category took); everything else is spread over the 64 lanes:
//   * lane l = a * T + t owns one (area range, IoU threshold) pair through the whole image: its matched set is a bitset over
//     the ground truths in LDS (word w of lane l at s_gtm[w * 64 + l]: every lane reads and writes only its own words);
//   * the ground truths are laid out in LDS sorted by category, annotation order inside one (a rank count, once per image), so
//     a detection's candidates are one contiguous range, the same for every detection of the category;
//   * per detection the lanes first form the IoU row over that range (one ground truth per lane), then every lane walks the
//     row ONCE with its own ignore flags and threshold, keeping the best counted and the best ignored candidate apart: the
//     definition visits the counted ones first and looks at the ignored ones only when none of them matched, and the two
//     chains never read each other's running IoU;
//   * __ballot over "matched" / "ignored" IS the output word: bit a * T + t of match[b, d] / ignore[b, d].
// Categories never meet, so visiting the detections in one global (score descending, index ascending) order gives every
// category its own stable descending order.  fp64 throughout after the detection's fp32 w = x2 - x1, h = y2 - y1; built with
// -ffp-contract=off (w * h, da + ga - inter round like the host's doubles; the division is IEEE).  No atomics, vector stores
// only, every output element is written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"

#define CM_THREADS 64
#define CM_MAX_D 100               // include/sfod_hip.h, evaluation.py COCO_DET_CAP (MAX_DETS[-1])
#define CM_MAX_G 256               // include/sfod_hip.h, evaluation.py COCO_GT_CAP
#define CM_MAX_AT 64               // one lane, one output bit per (area range, threshold)
#define CM_GT_WORDS (CM_MAX_G / 32)

struct CocoMatchArgs {             // by value in the launch arguments, like MosaicArgs
  double thr[CM_MAX_AT];           // IOU_THRS as the host holds them, never recomputed here
  double lo[CM_MAX_AT], hi[CM_MAX_AT];
  int B, D, G, K, A, T;
};

// Python's min(a, b) / max(a, b) on floats: the first argument unless the second is strictly smaller / larger
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }

// does detection i come before detection j in numpy's stable argsort of -score?  (a NaN ranks behind every number)
__device__ __forceinline__ bool cm_before(float si, int i, float sj, int j) {
  const bool ni = si != si, nj = sj != sj;
  if (ni || nj) return (ni && nj) ? i < j : nj;
  return si > sj || (si == sj && i < j);
}

__global__ void __launch_bounds__(CM_THREADS)
k_coco_match(const CocoMatchArgs p, const float* __restrict__ dboxes, const float* __restrict__ dscores,
             const int32_t* __restrict__ dcls, const int32_t* __restrict__ dcount, const double* __restrict__ gboxes,
             const double* __restrict__ garea, const int32_t* __restrict__ gcls, const int32_t* __restrict__ gcrowd,
             const int32_t* __restrict__ gcount, int32_t* __restrict__ rank, uint64_t* __restrict__ match,
             uint64_t* __restrict__ ignore, int32_t* __restrict__ npig) {
  __shared__ double s_dx[CM_MAX_D], s_dy[CM_MAX_D], s_dw[CM_MAX_D], s_dh[CM_MAX_D];
  __shared__ float s_ds[CM_MAX_D];
  __shared__ int s_dc[CM_MAX_D], s_order[CM_MAX_D], s_lo[CM_MAX_D], s_hi[CM_MAX_D];
  __shared__ int s_raw[CM_MAX_G];              // categories in annotation order (the sort's input)
  __shared__ double s_gx[CM_MAX_G], s_gy[CM_MAX_G], s_gw[CM_MAX_G], s_gh[CM_MAX_G];   // from here on: sorted by category
  __shared__ int s_gc[CM_MAX_G];
  __shared__ uint32_t s_gf[CM_MAX_G];          // bit a: ignored in area range a; bit 31: crowd
  __shared__ double s_iou[CM_MAX_G];           // the current detection's row over its category's range
  __shared__ uint32_t s_gtm[CM_GT_WORDS * CM_THREADS];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int D = p.D, G = p.G, K = p.K, A = p.A, T = p.T;
  const int nd = min(max(dcount[b], 0), D), ng = min(max(gcount[b], 0), G);

  for (int d = lane; d < nd; d += CM_THREADS) {            // a slot at or beyond the count is never read
    const float4 v = *reinterpret_cast<const float4*>(dboxes + ((int64_t)b * D + d) * 4);
    const float w = v.z - v.x, h = v.w - v.y;              // fp32, as instances_to_coco_json subtracts
    s_dx[d] = (double)v.x; s_dy[d] = (double)v.y; s_dw[d] = (double)w; s_dh[d] = (double)h;
    s_ds[d] = dscores[(int64_t)b * D + d];
    s_dc[d] = dcls[(int64_t)b * D + d];
  }
  for (int g = lane; g < ng; g += CM_THREADS) s_raw[g] = gcls[(int64_t)b * G + g];
  for (int w = 0; w < CM_GT_WORDS; ++w) s_gtm[w * CM_THREADS + lane] = 0u;
  __syncthreads();
  for (int g = lane; g < ng; g += CM_THREADS) {
    const int c = s_raw[g];
    int at = 0;                                            // stable: by category, then annotation order
    for (int e = 0; e < ng; ++e) at += s_raw[e] < c || (s_raw[e] == c && e < g);
    const int64_t o = (int64_t)b * G + g;
    s_gx[at] = gboxes[o * 4]; s_gy[at] = gboxes[o * 4 + 1]; s_gw[at] = gboxes[o * 4 + 2]; s_gh[at] = gboxes[o * 4 + 3];
    s_gc[at] = c;
    const double ar = garea[o];
    const bool crowd = gcrowd[o] != 0;
    uint32_t f = crowd ? 0x80000000u : 0u;
    for (int a = 0; a < A; ++a)
      if (crowd || ar < p.lo[a] || ar > p.hi[a]) f |= 1u << a;
    s_gf[at] = f;
  }
  __syncthreads();

  // rank inside the category (the output), the global visiting order and the category's range of ground truths
  for (int d = lane; d < D; d += CM_THREADS) {
    int r = -1;
    if (d < nd && s_dc[d] >= 0 && s_dc[d] < K) {
      const float s = s_ds[d];
      const int c = s_dc[d];
      int same = 0, all = 0;
      for (int e = 0; e < nd; ++e) {
        const int ce = s_dc[e];
        if (e == d || ce < 0 || ce >= K) continue;
        const bool bf = cm_before(s_ds[e], e, s, d);
        all += bf;
        same += bf && ce == c;
      }
      r = same;
      s_order[all] = d;
      int lt = 0, le = 0;
      for (int g = 0; g < ng; ++g) {
        lt += s_gc[g] < c;
        le += s_gc[g] <= c;
      }
      s_lo[d] = lt;
      s_hi[d] = le;
    }
    rank[(int64_t)b * D + d] = r;
    if (r < 0) {                                            // beyond the count or outside [0, K): in no category
      match[(int64_t)b * D + d] = 0ull;
      ignore[(int64_t)b * D + d] = 0ull;
    }
  }
  int nvalid = 0;
  for (int d = lane; d < nd; d += CM_THREADS) nvalid += s_dc[d] >= 0 && s_dc[d] < K;
  nvalid = wave_sum_i(nvalid);

  // ground truths that count, per (category, area range)
  for (int j = lane; j < K * A; j += CM_THREADS) {
    const int k = j / A, a = j - k * A;
    int n = 0;
    for (int g = 0; g < ng; ++g) n += s_gc[g] == k && !((s_gf[g] >> a) & 1u);
    npig[(int64_t)b * K * A + j] = n;
  }
  __syncthreads();

  const bool live = lane < A * T;
  const int a = live ? lane / T : 0;
  const double t0 = live ? p.thr[lane - a * T] : 0.0;
  const double lo = p.lo[a], hi = p.hi[a];
  const double start = py_min(t0, 1 - 1e-10);
  for (int q = 0; q < nvalid; ++q) {
    const int d = s_order[q];
    const int g_lo = s_lo[d], g_hi = s_hi[d];               // this category's ground truths, annotation order
    const double dx = s_dx[d], dy = s_dy[d], dw = s_dw[d], dh = s_dh[d];
    const double da = dw * dh;
    for (int g = g_lo + lane; g < g_hi; g += CM_THREADS) {
      const double gx = s_gx[g], gy = s_gy[g], gw = s_gw[g], gh = s_gh[g];
      const double w = py_min(dx + dw, gx + gw) - py_max(dx, gx);
      const double h = py_min(dy + dh, gy + gh) - py_max(dy, gy);
      double v = 0.0;
      if (!(w <= 0 || h <= 0)) {
        const double inter = w * h;
        v = inter / ((s_gf[g] >> 31) ? da : (da + gw * gh) - inter);
      }
      s_iou[g - g_lo] = v;
    }
    __syncthreads();
    double iou0 = start, iou1 = start;                      // the running IoU of the counted / the ignored candidates
    int m0 = -1, m1 = -1;
    if (live && g_lo < g_hi) {
      for (int w = g_lo >> 5; w <= (g_hi - 1) >> 5; ++w) {
        const uint32_t taken = s_gtm[w * CM_THREADS + lane];
        const int g_end = min(g_hi, (w + 1) << 5);
#pragma unroll 4
        for (int g = max(g_lo, w << 5); g < g_end; ++g) {
          const uint32_t f = s_gf[g];
          const double v = s_iou[g - g_lo];
          if (((taken >> (g & 31)) & 1u) && !(f >> 31)) continue;     // already matched and not crowd
          if ((f >> a) & 1u) {
            if (v < iou1) continue;
            iou1 = v;
            m1 = g;
          } else {
            if (v < iou0) continue;
            iou0 = v;
            m0 = g;
          }
        }
      }
    }
    const bool counted = m0 > -1;                           // a counted match stands; ignored ones are looked at without one
    const int mg = counted ? m0 : m1;
    if (mg > -1) s_gtm[(mg >> 5) * CM_THREADS + lane] |= 1u << (mg & 31);
    const bool out_of_range = da < lo || da > hi;
    const uint64_t mm = __ballot(live && mg > -1);
    const uint64_t ii = __ballot(live && (mg > -1 ? !counted : out_of_range));
    if (lane == 0) {
      match[(int64_t)b * D + d] = mm;
      ignore[(int64_t)b * D + d] = ii;
    }
    __syncthreads();                                        // the row is rewritten by the next detection
  }
}

extern "C" int sfod_coco_match(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                               const int32_t* det_count, const double* gt_boxes, const double* gt_area,
                               const int32_t* gt_classes, const int32_t* gt_iscrowd, const int32_t* gt_count, int B, int D,
                               int G, int K, const double* iou_thrs, int T, const double* area_rng, int A, int32_t* rank,
                               uint64_t* match, uint64_t* ignore, int32_t* npig, void* stream) {
  SFOD_REQUIRE_EXTENTS("coco_match", B, D, G, K, T, A);
  SFOD_REQUIRE(A >= 1 && T >= 1 && A <= CM_MAX_AT && T <= CM_MAX_AT && A * T <= CM_MAX_AT,
               "coco_match: A >= 1, T >= 1 and A * T <= 64 (one output bit per area range and threshold)");
  SFOD_REQUIRE(D >= 1 && D <= CM_MAX_D, "coco_match: D must be in 1..100 (TEST.DETECTIONS_PER_IMAGE, COCOeval's maxDets)");
  SFOD_REQUIRE(G >= 1 && G <= CM_MAX_G, "coco_match: G must be in 1..256 (the ground-truth cap)");
  SFOD_REQUIRE(K >= 1, "coco_match: K must be positive");
  SFOD_REQUIRE(sfod_prod_fits({B, K, A}), "coco_match: oversized npig");
  SFOD_REQUIRE(det_boxes != nullptr && det_scores != nullptr && det_classes != nullptr && det_count != nullptr &&
                   gt_boxes != nullptr && gt_area != nullptr && gt_classes != nullptr && gt_iscrowd != nullptr &&
                   gt_count != nullptr && iou_thrs != nullptr && area_rng != nullptr && rank != nullptr &&
                   match != nullptr && ignore != nullptr && npig != nullptr,
               "coco_match: null argument");
  CocoMatchArgs p;
  for (int i = 0; i < CM_MAX_AT; ++i) p.thr[i] = p.lo[i] = p.hi[i] = 0.0;
  for (int t = 0; t < T; ++t) {
    SFOD_REQUIRE(isfinite(iou_thrs[t]), "coco_match: a threshold is not finite");
    p.thr[t] = iou_thrs[t];
  }
  for (int a = 0; a < A; ++a) {
    SFOD_REQUIRE(isfinite(area_rng[2 * a]) && isfinite(area_rng[2 * a + 1]), "coco_match: an area range is not finite");
    p.lo[a] = area_rng[2 * a];
    p.hi[a] = area_rng[2 * a + 1];
  }
  p.B = B; p.D = D; p.G = G; p.K = K; p.A = A; p.T = T;
  if (B == 0) return 0;
  hipLaunchKernelGGL(k_coco_match, dim3(B), dim3(CM_THREADS), 0, (hipStream_t)stream, p, det_boxes, det_scores,
                     det_classes, det_count, gt_boxes, gt_area, gt_classes, gt_iscrowd, gt_count, rank, match, ignore, npig);
  return sfod_check_launch("coco_match");
}
