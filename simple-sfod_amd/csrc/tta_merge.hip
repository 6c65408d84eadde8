// TEST.AUG (Detectron2's GeneralizedRCNNWithTTA): the step between the augmented passes and the class-wise NMS.
//
// Every pass leaves its detections in the fixed-capacity containers of sfod_frcnn_finalize.  sfod_tta_merge takes the
// containers of B images x A augmentations back to the original frame (d2 `_get_augmented_boxes`: the inverse transform
// list in reverse order, each transform's apply_box on the corners with min / max, float32 throughout), concatenates them
// in augmentation order and applies the entry of fast_rcnn_inference_single_image (`_merge_detections`): non-finite rows
// dropped, clip to (H0, W0), score > thresh (strict).  It writes the COMPACT candidate arrays -- one slot per detection,
// its class beside it -- that sfod_segmented_sort_desc -> sfod_frcnn_prepare_nms_cls -> sfod_nms -> sfod_frcnn_finalize
// consume.  One thread owns one candidate, one workgroup one image; cand_count is a workgroup sum of integers in fixed
// order (no atomics).  Built with -ffp-contract=off: w_a - x and the two multiplications round like numpy's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"

#define TTA_THREADS 256
#define TTA_MAX_AUG 64
#define TTA_MAX_CAND 4096          // A * cap: include/sfod_hip.h, modeling/tta_options.py MERGE_CAPACITY
#define TTA_ROW 8                  // floats per (image, augmentation) table row

__global__ void __launch_bounds__(TTA_THREADS)
k_tta_merge(const float* __restrict__ dboxes, const float* __restrict__ dscores, const int32_t* __restrict__ dcls,
            const int32_t* __restrict__ dcount, const float* __restrict__ table, const int32_t* __restrict__ sizes,
            int A, int cap, int K, float thr, float* __restrict__ cboxes, float* __restrict__ cscores,
            int32_t* __restrict__ ccls, int32_t* __restrict__ ccount) {
  __shared__ int s_wave[TTA_THREADS / 64];
  const int b = blockIdx.x;
  const int n = A * cap;
  const float H0 = (float)sizes[b * 2], W0 = (float)sizes[b * 2 + 1];
  int npass = 0;
  for (int j = threadIdx.x; j < n; j += TTA_THREADS) {
    const int a = j / cap, i = j - a * cap;
    const int64_t row = (int64_t)b * A + a;
    const int64_t src = row * cap + i;
    const int live_n = min(max(dcount[row], 0), cap);
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, sc = -1.f;
    int c = 0;
    bool pass = false;
    if (i < live_n) {                        // a slot at or beyond det_count is never read
      const float4 v = *reinterpret_cast<const float4*>(dboxes + src * 4);
      const float s = dscores[src];
      c = dcls[src];
      const float* t = table + row * TTA_ROW;       // (w_a, h_a, flip, w / w_a, h / h_a, W0 / w, H0 / h, unused)
      const float wa = t[0], rx1 = t[3], ry1 = t[4], rx2 = t[5], ry2 = t[6];
      bool fin = isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w) && isfinite(s);
      float ax = v.x, bx = v.z, ay = v.y, by = v.w;
      if (t[2] != 0.f) { ax = wa - v.x; bx = wa - v.z; }                    // HFlipTransform(w_a).apply_coords
      x1 = fminf(ax, bx); x2 = fmaxf(ax, bx); y1 = fminf(ay, by); y2 = fmaxf(ay, by);
      ax = x1 * rx1; bx = x2 * rx1; ay = y1 * ry1; by = y2 * ry1;           // ResizeTransform(h_a, w_a -> h, w)
      x1 = fminf(ax, bx); x2 = fmaxf(ax, bx); y1 = fminf(ay, by); y2 = fmaxf(ay, by);
      ax = x1 * rx2; bx = x2 * rx2; ay = y1 * ry2; by = y2 * ry2;           // ResizeTransform(h, w -> H0, W0)
      x1 = fminf(ax, bx); x2 = fmaxf(ax, bx); y1 = fminf(ay, by); y2 = fmaxf(ay, by);
      // (numpy's min / max hand a NaN on, fminf / fmaxf drop it: the input's own finite test stands for that)
      fin = fin && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
      pass = fin && c >= 0 && c < K && (s > thr);
      if (pass) {
        x1 = fminf(fmaxf(x1, 0.f), W0); x2 = fminf(fmaxf(x2, 0.f), W0);
        y1 = fminf(fmaxf(y1, 0.f), H0); y2 = fminf(fmaxf(y2, 0.f), H0);
        sc = s;
      }
    }
    const int64_t o = (int64_t)b * n + j;
    *reinterpret_cast<float4*>(cboxes + o * 4) = pass ? make_float4(x1, y1, x2, y2) : make_float4(0.f, 0.f, 0.f, 0.f);
    cscores[o] = sc;
    ccls[o] = pass ? c : 0;
    npass += pass;
  }
  npass = wave_sum_i(npass);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = npass;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < TTA_THREADS / 64; ++w) tot += s_wave[w];
    ccount[b] = tot;
  }
}

extern "C" int sfod_tta_merge(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                              const int32_t* det_count, const float* aug_table, const int32_t* image_sizes, int B,
                              int A, int cap, int K, float score_thresh, float* cand_boxes, float* cand_scores,
                              int32_t* cand_classes, int32_t* cand_count, void* stream) {
  SFOD_REQUIRE_EXTENTS("tta_merge", B, A, cap, K);
  SFOD_REQUIRE(A >= 1 && A <= TTA_MAX_AUG, "tta_merge: A must be in 1..64");
  SFOD_REQUIRE(cap >= 1 && cap <= TTA_MAX_CAND && A * cap <= TTA_MAX_CAND, "tta_merge: cap >= 1 and A * cap <= 4096");
  SFOD_REQUIRE(K >= 1, "tta_merge: K must be positive");
  SFOD_REQUIRE(B >= 1 && B <= 65535, "tta_merge: B must be in 1..65535");
  SFOD_REQUIRE(isfinite(score_thresh), "tta_merge: score_thresh must be finite");
  SFOD_REQUIRE(det_boxes != nullptr && det_scores != nullptr && det_classes != nullptr && det_count != nullptr &&
                   aug_table != nullptr && image_sizes != nullptr && cand_boxes != nullptr && cand_scores != nullptr &&
                   cand_classes != nullptr && cand_count != nullptr,
               "tta_merge: null argument");
  hipLaunchKernelGGL(k_tta_merge, dim3(B), dim3(TTA_THREADS), 0, (hipStream_t)stream, det_boxes, det_scores, det_classes,
                     det_count, aug_table, image_sizes, A, cap, K, score_thresh, cand_boxes, cand_scores, cand_classes,
                     cand_count);
  return sfod_check_launch("tta_merge");
}
