// Mosaic composition on the device (TRAINER base_mosaic / base_mosaic_wq / base_mosaic_wq_new; daod/data/mappers/mosaic.py:81-265):
// up to four uint8 [3][h0][w0] tiles are scaled up to their native size (Pillow-exact bilinear, the arithmetic of
// k_resize_bilinear_u8 in elementwise.hip bit for bit: 22-bit coefficients, round + clip to uint8 between the horizontal and the
// vertical pass), pasted into a [2*H0][2*W0] canvas filled with `fill`, and the canvas is halved with the rounded 2x2 mean --
// in ONE launch.  Neither the canvas nor an up-scaled tile exists in memory: a workgroup owns a 16 x 64 output tile = 32 x 128
// canvas pixels, which it composes in LDS (fill, then tile after tile in paste order, so a later tile overwrites an earlier
// one) and reduces.  Per tile that touches the block: phase A writes the horizontally filtered source rows the block needs, at
// the block's canvas columns, into LDS once; phase B filters them vertically.  Rectangle edges are handled per canvas pixel:
// an odd paste offset (a letterboxed tile) mixes fill and image inside one 2x2 cell.  No atomics; HBM traffic is the tiles
// once (plus halo rows) and the output once.
#include "common.h"

namespace {

constexpr int MS_PREC = 22;
constexpr int MS_TH = 16, MS_TW = 64;                 // output tile of a workgroup
constexpr int MS_CH = 2 * MS_TH, MS_CW = 2 * MS_TW;   // its canvas block
constexpr int MS_ROWS = 40;                           // horizontally filtered source rows held in LDS (32 * h0 / h + taps)
constexpr int MS_MAX_TILES = 4;
constexpr int MS_GEOM = 14;                           // ints per tile in the host geometry array

__device__ __forceinline__ int ms_clip8(int v) {
  v >>= MS_PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct MosaicTile {
  const uint8_t* src;        // [3][h0][w0]
  const int32_t* htab;       // bounds int32 [w][2] followed by coefficients int32 [w][ksh]; nullptr: identity scale
  const int32_t* vtab;       // the same for h / ksv
  int h0, w0, h, w;          // mapped size, up-scaled size
  int lx1, ly1, lx2, ly2;    // paste rectangle on the canvas
  int sx1, sy1;              // its origin in the up-scaled tile
  int ksh, ksv;
};

struct MosaicArgs {
  MosaicTile t[MS_MAX_TILES];
  int n, H0, W0, fill, tiles_x, wide;
};

__global__ void __launch_bounds__(256)
k_mosaic_u8(const MosaicArgs a, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(8))) uint8_t cv[3][MS_CH][MS_CW];
  __shared__ uint8_t tmp[3][MS_ROWS][MS_CW];
  __shared__ int s_r0[MS_CH], s_kv[MS_CH][4];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int cy0 = ty * MS_CH, cx0 = tx * MS_CW;
  {
    uint32_t* cv32 = reinterpret_cast<uint32_t*>(&cv[0][0][0]);
    const uint32_t f4 = (uint32_t)a.fill * 0x01010101u;
    for (int i = tid; i < 3 * MS_CH * MS_CW / 4; i += 256) cv32[i] = f4;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < MS_MAX_TILES; ++k) {
    if (k >= a.n) break;
    const MosaicTile& t = a.t[k];
    // the part of the paste rectangle inside this block (canvas coordinates); every condition below is uniform in the block
    const int ya = max(cy0, t.ly1), yb = min(cy0 + MS_CH, t.ly2);
    const int xa = max(cx0, t.lx1), xb = min(cx0 + MS_CW, t.lx2);
    if (ya >= yb || xa >= xb) continue;
    const int64_t plane = (int64_t)t.h0 * t.w0;
    const int dy = t.sy1 - t.ly1, dx = t.sx1 - t.lx1;      // canvas -> up-scaled tile
    if (t.htab == nullptr) {
      // ---- identity scale: the tile is already at canvas scale (base_mosaic_wq_new, or mapped == native) -----------------
      for (int g = tid; g < MS_CH * (MS_CW / 4); g += 256) {
        const int cyl = g / (MS_CW / 4), cxl = (g - cyl * (MS_CW / 4)) * 4;
        const int cy = cy0 + cyl, cx = cx0 + cxl;
        if (cy < ya || cy >= yb || cx + 4 <= xa || cx >= xb) continue;
        const int64_t row = (int64_t)(cy + dy) * t.w0 + dx;
        if (cx >= xa && cx + 4 <= xb) {                    // four pixels of one row of the tile: inside the tensor
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            uint32_t v;
            __builtin_memcpy(&v, t.src + c * plane + row + cx, 4);
            *reinterpret_cast<uint32_t*>(&cv[c][cyl][cxl]) = v;
          }
        } else {
          for (int i = 0; i < 4; ++i)
            if (cx + i >= xa && cx + i < xb)
              for (int c = 0; c < 3; ++c) cv[c][cyl][cxl + i] = t.src[c * plane + row + cx + i];
        }
      }
      __syncthreads();
      continue;
    }
    const int32_t* hb = t.htab;
    const int32_t* hk = t.htab + 2 * (int64_t)t.w;
    const int32_t* vb = t.vtab;
    const int32_t* vk = t.vtab + 2 * (int64_t)t.h;
    const int uya = ya + dy, uyb = yb - 1 + dy;            // first / last row of the up-scaled tile in this block
    const int rmin = min(max(vb[2 * uya], 0), t.h0 - 1);
    const int nrows = vb[2 * uyb] + vb[2 * uyb + 1] - rmin;
    if (nrows <= MS_ROWS && t.ksh <= 4 && t.ksv <= 4 && 3 * plane >= 4) {
      // the vertical taps of the block's canvas rows, read from the table once (phase B then touches LDS only)
      if (tid < MS_CH) {
        const int cy = cy0 + tid;
        if (cy >= ya && cy < yb) {
          const int uy = cy + dy;
          const int yn = min(vb[2 * uy + 1], t.ksv);
          s_r0[tid] = vb[2 * uy] - rmin;
#pragma unroll
          for (int j = 0; j < 4; ++j) s_kv[tid][j] = (j < yn) ? vk[(int64_t)uy * t.ksv + j] : 0;
        }
      }
      // ---- phase A: thread = (canvas column, row group); the column's taps are loaded once -------------------------------
      {
        const int cxl = tid & (MS_CW - 1), rg = tid / MS_CW;
        const int cx = cx0 + cxl;
        if (cx >= xa && cx < xb) {
          const int ux = cx + dx;
          const int xmin = min(max(hb[2 * ux], 0), t.w0 - 1);
          const int xn = min(min(hb[2 * ux + 1], t.ksh), t.w0 - xmin);
          int kh[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) kh[i] = (i < xn) ? hk[(int64_t)ux * t.ksh + i] : 0;
          // INVARIANT: the 4-byte tap load stays inside the TENSOR -- lim is the last legal start in the whole [3,h0,w0] tile;
          // at the tensor's very end the load is shifted left (the taps beyond carry weight 0)
          const int64_t lim = 3 * plane - 4;
#pragma unroll 4
          for (int r = rg; r < nrows; r += 256 / MS_CW) {
            const int64_t off = (int64_t)min(rmin + r, t.h0 - 1) * t.w0 + xmin;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const int64_t at = c * plane + off;
              const int64_t o2 = at <= lim ? at : lim;
              uint32_t v;
              __builtin_memcpy(&v, t.src + o2, 4);
              v >>= (int)(at - o2) * 8;
              int sh = 1 << (MS_PREC - 1);
#pragma unroll
              for (int i = 0; i < 4; ++i) sh += (int)((v >> (8 * i)) & 0xffu) * kh[i];
              tmp[c][r][cxl] = (uint8_t)ms_clip8(sh);
            }
          }
        }
      }
      __syncthreads();
      // ---- phase B: thread = canvas pixels (column, row group + 2 k) ------------------------------------------------------
      {
        const int cxl = tid & (MS_CW - 1), rg = tid / MS_CW;
        const int cx = cx0 + cxl;
        if (cx >= xa && cx < xb) {
#pragma unroll 2
          for (int cy = ya + rg; cy < yb; cy += 256 / MS_CW) {
            const int cyl = cy - cy0;
            const int r0 = s_r0[cyl];
            int kv[4], rr[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              kv[j] = s_kv[cyl][j];
              rr[j] = min(max(r0 + j, 0), MS_ROWS - 1);          // (rows beyond the taps carry weight 0)
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              int acc = 1 << (MS_PREC - 1);
#pragma unroll
              for (int j = 0; j < 4; ++j) acc += (int)tmp[c][rr[j]][cxl] * kv[j];
              cv[c][cyl][cxl] = (uint8_t)ms_clip8(acc);
            }
          }
        }
      }
      __syncthreads();
    } else {
      // ---- generic body (a strongly down-scaled tile: more rows or taps than the LDS form holds): both passes per pixel ----
      for (int g = tid; g < MS_CH * MS_CW; g += 256) {
        const int cyl = g / MS_CW, cxl = g - cyl * MS_CW;
        const int cy = cy0 + cyl, cx = cx0 + cxl;
        if (cy < ya || cy >= yb || cx < xa || cx >= xb) continue;
        const int ux = cx + dx, uy = cy + dy;
        const int xmin = min(max(hb[2 * ux], 0), t.w0 - 1);
        const int xn = min(min(hb[2 * ux + 1], t.ksh), t.w0 - xmin);
        const int ymin = min(max(vb[2 * uy], 0), t.h0 - 1);
        const int yn = min(min(vb[2 * uy + 1], t.ksv), t.h0 - ymin);
        for (int c = 0; c < 3; ++c) {
          int acc = 1 << (MS_PREC - 1);
          for (int j = 0; j < yn; ++j) {
            const uint8_t* row = t.src + c * plane + (int64_t)(ymin + j) * t.w0 + xmin;
            int sh = 1 << (MS_PREC - 1);
            for (int i = 0; i < xn; ++i) sh += (int)row[i] * hk[(int64_t)ux * t.ksh + i];
            acc += ms_clip8(sh) * vk[(int64_t)uy * t.ksv + j];
          }
          cv[c][cyl][cxl] = (uint8_t)ms_clip8(acc);
        }
      }
      __syncthreads();
    }
  }
  // ---- the halving: rounded mean of each 2x2 canvas cell; thread = four output pixels of one row, one 4-byte store ---------
  {
    const int yl = tid / (MS_TW / 4), xl = (tid - yl * (MS_TW / 4)) * 4;
    const int y = ty * MS_TH + yl, x = tx * MS_TW + xl;
    if (y < a.H0 && x < a.W0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        uint64_t r0, r1;
        __builtin_memcpy(&r0, &cv[c][2 * yl][2 * xl], 8);
        __builtin_memcpy(&r1, &cv[c][2 * yl + 1][2 * xl], 8);
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int s = (int)((r0 >> (16 * i)) & 0xff) + (int)((r0 >> (16 * i + 8)) & 0xff) +
                        (int)((r1 >> (16 * i)) & 0xff) + (int)((r1 >> (16 * i + 8)) & 0xff);
          v |= (uint32_t)((s + 2) >> 2) << (8 * i);
        }
        uint8_t* d = out + ((int64_t)c * a.H0 + y) * a.W0 + x;
        if (a.wide && x + 4 <= a.W0) {
          *reinterpret_cast<uint32_t*>(d) = v;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (x + i < a.W0) d[i] = (uint8_t)(v >> (8 * i));
        }
      }
    }
  }
}

}  // namespace

extern "C" int sfod_mosaic_u8(const void* const* tiles, const void* const* tabs, const int32_t* geom, int n_tiles, int fill,
                              void* out, int H0, int W0, void* stream) {
  SFOD_REQUIRE_EXTENTS("mosaic_u8", n_tiles, fill, H0, W0);
  SFOD_REQUIRE(n_tiles >= 1 && n_tiles <= MS_MAX_TILES, "mosaic_u8: one to four tiles");
  SFOD_REQUIRE(fill <= 255, "mosaic_u8: fill outside [0, 255]");
  SFOD_REQUIRE(H0 >= 1 && W0 >= 1, "mosaic_u8: non-positive output extent");
  SFOD_REQUIRE(tiles != nullptr && tabs != nullptr && geom != nullptr, "mosaic_u8: tiles / tabs / geom are host arrays");
  SFOD_REQUIRE(out != nullptr, "mosaic_u8: NULL output");
  SFOD_REQUIRE(sfod_prod_fits({3, H0, W0}, 1LL << 38), "mosaic_u8: oversized output");
  SFOD_REQUIRE(sfod_prod_fits({(H0 + MS_TH - 1) / MS_TH, (W0 + MS_TW - 1) / MS_TW}), "mosaic_u8: too many workgroups");
  MosaicArgs a;
  for (int k = 0; k < MS_MAX_TILES; ++k) a.t[k] = MosaicTile{};
  for (int k = 0; k < n_tiles; ++k) {
    const int32_t* g = geom + k * MS_GEOM;
    const int h0 = g[0], w0 = g[1], h = g[2], w = g[3], lx1 = g[4], ly1 = g[5], lx2 = g[6], ly2 = g[7];
    const int sx1 = g[8], sy1 = g[9], sx2 = g[10], sy2 = g[11], ksh = g[12], ksv = g[13];
    SFOD_REQUIRE(sfod_ints_ok({h0, w0, h, w, lx1, ly1, lx2, ly2, sx1, sy1, sx2, sy2, ksh, ksv}),
                 "mosaic_u8: negative or oversized tile geometry");
    SFOD_REQUIRE(h0 >= 1 && w0 >= 1 && h >= 1 && w >= 1, "mosaic_u8: non-positive tile extent");
    SFOD_REQUIRE(sfod_prod_fits({3, h0, w0}, 1LL << 38) && sfod_prod_fits({h, 16}) && sfod_prod_fits({w, 16}),
                 "mosaic_u8: oversized tile");
    SFOD_REQUIRE(tiles[k] != nullptr, "mosaic_u8: NULL tile");
    SFOD_REQUIRE(lx1 <= lx2 && ly1 <= ly2 && (int64_t)lx2 <= 2 * (int64_t)W0 && (int64_t)ly2 <= 2 * (int64_t)H0,
                 "mosaic_u8: a paste rectangle leaves the canvas");
    SFOD_REQUIRE(sx1 <= sx2 && sy1 <= sy2 && sx2 <= w && sy2 <= h, "mosaic_u8: a source rectangle leaves its tile");
    SFOD_REQUIRE(sx2 - sx1 == lx2 - lx1 && sy2 - sy1 == ly2 - ly1, "mosaic_u8: paste and source rectangle differ in extent");
    const bool identity = tabs[2 * k] == nullptr && tabs[2 * k + 1] == nullptr;
    if (identity) {
      SFOD_REQUIRE(h == h0 && w == w0, "mosaic_u8: a tile without coefficient tables must be at canvas scale");
    } else {
      SFOD_REQUIRE(tabs[2 * k] != nullptr && tabs[2 * k + 1] != nullptr, "mosaic_u8: one coefficient table of a tile is NULL");
      SFOD_REQUIRE(ksh >= 1 && ksv >= 1 && sfod_prod_fits({w, ksh}) && sfod_prod_fits({h, ksv}), "mosaic_u8: bad tap count");
    }
    MosaicTile& t = a.t[k];
    t.src = (const uint8_t*)tiles[k];
    t.htab = (const int32_t*)tabs[2 * k];
    t.vtab = (const int32_t*)tabs[2 * k + 1];
    t.h0 = h0, t.w0 = w0, t.h = h, t.w = w;
    t.lx1 = lx1, t.ly1 = ly1, t.lx2 = lx2, t.ly2 = ly2, t.sx1 = sx1, t.sy1 = sy1;
    t.ksh = ksh, t.ksv = ksv;
  }
  a.n = n_tiles, a.H0 = H0, a.W0 = W0, a.fill = fill;
  a.tiles_x = (W0 + MS_TW - 1) / MS_TW;
  a.wide = ((W0 & 3) == 0 && ((uintptr_t)out & 3) == 0) ? 1 : 0;
  const int tiles_y = (H0 + MS_TH - 1) / MS_TH;
  hipLaunchKernelGGL(k_mosaic_u8, dim3(a.tiles_x * tiles_y), dim3(256), 0, (hipStream_t)stream, a, (uint8_t*)out);
  return sfod_check_launch("mosaic_u8");
}
