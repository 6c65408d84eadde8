// First VGG layer (conv1_1: 3 -> 64 channels, 3x3, pad 1) on bf16 MFMA, gfx950.
//
// The input has 3 real channels padded to one 16-byte chunk (8 bf16), so an im2col row is 9 taps x 8
// channels = 72 values and the layer is bound by writing its 64-channel output, not by arithmetic.  The
// generic implicit GEMM spends 0.48 ms on it (per-lane tap decoding, 128-row tiles, half-empty K tiles).
// Here: workgroup = 8 x 32 output pixels, 4 waves (two image rows each); the 10 x 34 halo patch is staged
// in LDS as one 16-byte chunk per pixel, so an A fragment of k-step s (taps 2s, 2s+1) is ONE conflict-free
// ds_read_b128 per lane; all ten weight fragments live in registers for the whole (grid-stride) tile loop.
// Epilogue as in conv3x3_patch.hip: bias, per-wave LDS staging for 16-byte stores, BatchNorm (sum, M2,
// count) per workgroup.
#include "conv_internal.h"
#include <type_traits>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace {

constexpr int TH = 8, TW = 32, PW = TW + 2, PH = TH + 2;
constexpr int PATCH_BYTES = PH * PW * 16;            // 5440
constexpr int STG_OFF = 5632;                        // staged C tiles: 4 waves x 64 rows x 144 B
constexpr int STG_PITCH = 144;
constexpr int SRED_OFF = STG_OFF + 4 * 64 * STG_PITCH;   // float [4][64][2] + float [4]
constexpr int LDS_BYTES = SRED_OFF + 4 * 64 * 2 * 4 + 16;
// SFOD_BF16X3 variant: 32-byte pixels ((8 hi | 8 lo) pairs), fp32 staging of 32 rows x 64 columns per wave (272-byte pitch)
constexpr int X3_PATCH_BYTES = PH * PW * 32;         // 10880
constexpr int X3_W_OFF = 11008;                      // weight fragments [k-step][j][hi/lo][lane] x 16 B (held in LDS, not
constexpr int X3_W_BYTES = 5 * 2 * 2 * 64 * 16;      // in 80 VGPRs: 3 workgroups per CU instead of 1)
constexpr int X3_STG_OFF = X3_W_OFF + X3_W_BYTES;
constexpr int X3_FP = 272;
constexpr int X3_SRED_OFF = X3_STG_OFF + 4 * 16 * X3_FP;   // 16 rows x 64 columns per wave at a time
constexpr int X3_SRED_BYTES = 4 * 64 * 2 * 4 + 16;
constexpr int X3_LDS_BYTES = X3_SRED_OFF + X3_SRED_BYTES;
// pipelined loop (f1_x3_pipe): two statistics buffers (tile n's partials are combined while tile n + 1 computes); the
// statistics-only pass, which stages no output, keeps a second patch buffer in the staging area.  Still 3 workgroups per CU.
constexpr int X3_PIPE_LDS_BYTES = X3_SRED_OFF + 2 * X3_SRED_BYTES;
static_assert(X3_PATCH_BYTES <= 4 * 16 * X3_FP, "the second patch buffer lives in the staging area");
static_assert(3 * X3_PIPE_LDS_BYTES <= 160 * 1024, "3 workgroups per CU");

// epilogue of the pipelined bf16x3 / f16x3 kernel, fixed per instantiation
enum { F1_PLAIN = 0, F1_STATS = 1, F1_Y = 2, F1_AFFINE = 3, F1_BN = 4 };

struct F1Args {
  const bf16_t* x;     // [B,H,W,8]   (bf16x3: 16 bf16 per pixel = 8 hi | 8 lo)
  const bf16_t* w;     // [64][9][8]  (bf16x3: 16 bf16 per (output channel, tap))
  const float* bias;
  const float* scale;  // optional per-channel affine applied to (conv + bias) before the activation: the BatchNorm
  const float* shift;  //   of a second pass whose statistics came from a first, store-free pass (teacher forward)
  void* y;             // [B,H,W,ldy] bf16 (bf16x3: fp32 without an affine, (hi, lo) pairs with one); nullptr: statistics only
  float* stats;
  int B, H, W, ldy, act;
  int tiles_y, tiles_x, ntiles;
  const unsigned* wamax;   // SFOD_F16X3: bits of max|w| of the scaled packed weights (common.h), or nullptr
  // F1_BN: z = relu(bn(conv + bias)) with sfod_bn_relu_pool_fwd's arithmetic (student pass 2: y itself came from pass 1)
  const float* mean;
  const float* invstd;
  const float* gamma;
  const float* beta;
};

__global__ void __launch_bounds__(256)
k_conv_first(F1Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5, l31 = lane & 31;

  // weight fragments: bq[j][s] = w[j*32 + l31][tap 2s+h][0..7], zeros for the padding tap 9
  bf16x8 bq[2][5];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int tap = 2 * s + h;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (tap < 9) v = *reinterpret_cast<const uint4*>(a.w + ((j * 32 + l31) * 9 + tap) * 8);
      bq[j][s] = __builtin_bit_cast(bf16x8, v);
    }
  float bcol[2], scol[2], hcol[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    bcol[j] = a.bias ? a.bias[j * 32 + l31] : 0.f;
    scol[j] = a.scale ? a.scale[j * 32 + l31] : 1.f;
    hcol[j] = a.shift ? a.shift[j * 32 + l31] : 0.f;
  }
  const float lo = (a.act == 1) ? 0.f : -__builtin_inff();

  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    int t = tile;
    const int txi = t % a.tiles_x;
    t /= a.tiles_x;
    const int tyi = t % a.tiles_y;
    const int b = t / a.tiles_y;
    const int x0 = txi * TW, y0 = tyi * TH;
    const bf16_t* ximg = a.x + (int64_t)b * a.H * a.W * 8;
    __syncthreads();   // previous tile's LDS users are done
    for (int p = threadIdx.x; p < PH * PW; p += 256) {
      const int py = p / PW, px = p - py * PW;
      const int iy = y0 - 1 + py, ix = x0 - 1 + px;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = *reinterpret_cast<const uint4*>(ximg + ((int64_t)iy * a.W + ix) * 8);
      *reinterpret_cast<uint4*>(smem + p * 16) = v;
    }
    __syncthreads();
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int tap = 2 * s + h;               // per-lane tap (two taps per k-step)
      const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = (2 * wave + i + ky) * PW + l31 + kx;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (tap < 9) v = *reinterpret_cast<const uint4*>(smem + row * 16);
        const bf16x8 af = __builtin_bit_cast(bf16x8, v);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bq[j][s], acc[i][j], 0, 0, 0);
      }
    }
    // ---- epilogue: rows of M-fragment i are the 32 pixels of image row y0 + 2*wave + i
    unsigned char* stg = smem + STG_OFF + wave * (64 * STG_PITCH);
    const bool full = (y0 + TH <= a.H) && (x0 + TW <= a.W);   // interior tile: no row masks
    unsigned vmask[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      unsigned m = 0xffffu;
      if (!full) {
        m = 0;
        const int iy = y0 + 2 * wave + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int px = (r & 3) + 8 * (r >> 2) + 4 * h;
          if (iy < a.H && x0 + px < a.W) m |= (1u << r);
        }
      }
      vmask[i] = m;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] += bcol[j];
    if (a.y != nullptr) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ml = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            // scol / hcol are (1, 0) without an affine and lo is -inf without a ReLU: two VALU ops per element,
            // no per-element select on the (uniform) mode
            const float o = fmaxf(__builtin_fmaf(acc[i][j][r], scol[j], hcol[j]), lo);
            *reinterpret_cast<bf16_t*>(stg + ml * STG_PITCH + (j * 32 + l31) * 2) = (bf16_t)o;
          }
      // same-wave readback (LDS is in order per wave): 8 rows x 128 B per instruction
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int row = it * 8 + (lane >> 3), ch = lane & 7;
        const int iy = y0 + 2 * wave + (row >> 5), ix = x0 + (row & 31);
        if (iy < a.H && ix < a.W) {
          const uint4 v = *reinterpret_cast<const uint4*>(stg + row * STG_PITCH + ch * 16);
          *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(a.y) + (((int64_t)b * a.H + iy) * a.W + ix) * a.ldy + ch * 8) = v;
        }
      }
    }
    if (a.stats != nullptr) {
      float* sred = reinterpret_cast<float*>(smem + SRED_OFF);   // [wave][64][2]
      float* scnt = sred + 4 * 64 * 2;
      int cnt = __builtin_popcount(vmask[0]) + __builtin_popcount(vmask[1]);
      cnt += __shfl_xor(cnt, 32);
      const float inv = 1.f / (float)(cnt > 0 ? cnt : 1);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float sm = 0.f, q = 0.f, mean;
        if (full) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) sm += acc[i][j][r];
          sm += __shfl_xor(sm, 32);
          mean = sm * inv;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float d = acc[i][j][r] - mean;
              q = __builtin_fmaf(d, d, q);
            }
        } else {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) sm += ((vmask[i] >> r) & 1u) ? acc[i][j][r] : 0.f;
          sm += __shfl_xor(sm, 32);
          mean = sm * inv;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float d = acc[i][j][r] - mean;
              q += ((vmask[i] >> r) & 1u) ? d * d : 0.f;
            }
        }
        q += __shfl_xor(q, 32);
        if (h == 0) {
          sred[(wave * 64 + j * 32 + l31) * 2 + 0] = sm;
          sred[(wave * 64 + j * 32 + l31) * 2 + 1] = q;
        }
      }
      if (lane == 0) scnt[wave] = (float)cnt;
      __syncthreads();
      if (threadIdx.x < 64) {
        const int col = threadIdx.x;
        double n_tot = 0.0, s_tot = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { n_tot += (double)scnt[k]; s_tot += (double)sred[(k * 64 + col) * 2]; }
        const double mu = n_tot > 0.0 ? s_tot / n_tot : 0.0;
        double m2 = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double nk = (double)scnt[k];
          if (nk > 0.0) {
            const double d = (double)sred[(k * 64 + col) * 2] / nk - mu;
            m2 += (double)sred[(k * 64 + col) * 2 + 1] + nk * d * d;
          }
        }
        a.stats[((int64_t)tile * 2 + 0) * 64 + col] = (float)s_tot;
        a.stats[((int64_t)tile * 2 + 1) * 64 + col] = (float)m2;
        if (col == 0) a.stats[(int64_t)a.ntiles * 2 * 64 + tile] = (float)n_tot;
      }
    }
  }
}

// ---- SFOD_BF16X3 variant ----------------------------------------------------------------------------------------------
// Same tiling; a k-step is (taps 2s, 2s+1) x 8 logical channels fed as hi*lo + lo*hi + hi*hi.  Output: fp32 y (student
// pass: the BatchNorm backward needs it), or -- with the affine of a second, recomputing pass (teacher) -- the next
// layer's operand pairs z = relu(scale * (conv + bias) + shift) directly; per wave 32 rows at a time are staged in LDS
// and stored as whole 256-byte pixels.
// f1_x3_plain is the loop as it was first written (SFOD_F1_PIPE=0): the reference f1_x3_pipe below is held to, bit for bit.
template <int FMT>      // 1: bf16 pairs (SFOD_BF16X3), 2: f16 pairs (SFOD_F16X3): MFMA opcode and the z pairs it writes
__device__ __forceinline__ void f1_x3_plain(const F1Args& a, unsigned char* smem) {
  using pair_t = typename std::conditional<FMT == 2, splith_t, split_t>::type;
  // SFOD_F16X3 weights carry a per-tensor power-of-two scale (common.h): undone on the accumulators (exact)
  const float winv = (FMT == 2 && a.wamax != nullptr) ? winv_from_absmax(*a.wamax) : 1.0f;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  // weight fragments -> LDS, once per workgroup (the grid is persistent)
  for (int e = threadIdx.x; e < 5 * 2 * 64; e += 256) {
    const int ln = e & 63, j = (e >> 6) & 1, ks = e >> 7;
    const int tap = 2 * ks + (ln >> 5);
    uint4 vh = make_uint4(0, 0, 0, 0), vl = vh;
    if (tap < 9) {
      const uint4* p = reinterpret_cast<const uint4*>(a.w + ((j * 32 + (ln & 31)) * 9 + tap) * 16);
      vh = p[0];
      vl = p[1];
    }
    *reinterpret_cast<uint4*>(smem + X3_W_OFF + (((ks * 2 + j) * 2 + 0) * 64 + ln) * 16) = vh;
    *reinterpret_cast<uint4*>(smem + X3_W_OFF + (((ks * 2 + j) * 2 + 1) * 64 + ln) * 16) = vl;
  }
  float bcol[2], scol[2], hcol[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    bcol[j] = a.bias ? a.bias[j * 32 + l31] : 0.f;
    scol[j] = a.scale ? a.scale[j * 32 + l31] : 1.f;
    hcol[j] = a.shift ? a.shift[j * 32 + l31] : 0.f;
  }
  const float lo = (a.act == 1) ? 0.f : -__builtin_inff();
  const bool zsplit = (a.scale != nullptr);

  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    int t = tile;
    const int txi = t % a.tiles_x;
    t /= a.tiles_x;
    const int tyi = t % a.tiles_y;
    const int b = t / a.tiles_y;
    const int x0 = txi * TW, y0 = tyi * TH;
    const bf16_t* ximg = a.x + (int64_t)b * a.H * a.W * 16;
    __syncthreads();   // previous tile's LDS users are done
    for (int p = threadIdx.x; p < PH * PW * 2; p += 256) {      // one 16-byte chunk (hi or lo) per thread and round
      const int pp = p >> 1, half = p & 1;
      const int py = pp / PW, px = pp - py * PW;
      const int iy = y0 - 1 + py, ix = x0 - 1 + px;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
        v = *reinterpret_cast<const uint4*>(ximg + ((int64_t)iy * a.W + ix) * 16 + half * 8);
      *reinterpret_cast<uint4*>(smem + p * 16) = v;
    }
    __syncthreads();
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int tap = 2 * s + h;
      const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = (2 * wave + i + ky) * PW + l31 + kx;
        uint4 vh = make_uint4(0, 0, 0, 0), vl = vh;
        if (tap < 9) {
          vh = *reinterpret_cast<const uint4*>(smem + row * 32);
          vl = *reinterpret_cast<const uint4*>(smem + row * 32 + 16);
        }
        const bf16x8 ah = __builtin_bit_cast(bf16x8, vh), al = __builtin_bit_cast(bf16x8, vl);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const bf16x8 bh = __builtin_bit_cast(
              bf16x8, *reinterpret_cast<const uint4*>(smem + X3_W_OFF + (((s * 2 + j) * 2 + 0) * 64 + lane) * 16));
          const bf16x8 bl = __builtin_bit_cast(
              bf16x8, *reinterpret_cast<const uint4*>(smem + X3_W_OFF + (((s * 2 + j) * 2 + 1) * 64 + lane) * 16));
          f32x16 c = acc[i][j];
          c = mfma_pairs<FMT>(ah, bl, c);
          c = mfma_pairs<FMT>(al, bh, c);
          c = mfma_pairs<FMT>(ah, bh, c);
          acc[i][j] = c;
        }
      }
    }
    const bool full = (y0 + TH <= a.H) && (x0 + TW <= a.W);
    unsigned vmask[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      unsigned m = 0xffffu;
      if (!full) {
        m = 0;
        const int iy = y0 + 2 * wave + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int px = (r & 3) + 8 * (r >> 2) + 4 * h;
          if (iy < a.H && x0 + px < a.W) m |= (1u << r);
        }
      }
      vmask[i] = m;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = acc[i][j][r] * winv + bcol[j];
    if (a.y != nullptr) {
      unsigned char* stg = smem + X3_STG_OFF + wave * (16 * X3_FP);
#pragma unroll
      for (int i = 0; i < 2; ++i) {          // M-fragment i = the 32 pixels of image row y0 + 2 * wave + i
        const int iy = y0 + 2 * wave + i;
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) {     // pixels 16 * qh .. 16 * qh + 15 (accumulator registers 8 * qh .. 8 * qh + 7)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
              const int r = qh * 8 + rr;
              const int ml = (rr & 3) + 8 * (rr >> 2) + 4 * h;
              const float o = fmaxf(__builtin_fmaf(acc[i][j][r], scol[j], hcol[j]), lo);
              *reinterpret_cast<float*>(stg + ml * X3_FP + (j * 32 + l31) * 4) = o;
            }
          if (zsplit) {
            // 8 lanes per pixel: 8 consecutive channels -> one 32-byte (hi | lo) group
#pragma unroll
            for (int it = 0; it < 2; ++it) {
              const int row = it * 8 + (lane >> 3), gch = lane & 7;
              const int ix = x0 + qh * 16 + row;
              if (iy < a.H && ix < a.W) {
                const float4 v0 = *reinterpret_cast<const float4*>(stg + row * X3_FP + gch * 32);
                const float4 v1 = *reinterpret_cast<const float4*>(stg + row * X3_FP + gch * 32 + 16);
                const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                split_store8(reinterpret_cast<pair_t*>(a.y) + (((int64_t)b * a.H + iy) * a.W + ix) * a.ldy + gch * 8, f);
              }
            }
          } else {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
              const int row = it * 4 + (lane >> 4), ch = lane & 15;
              const int ix = x0 + qh * 16 + row;
              if (iy < a.H && ix < a.W)
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.y) + (((int64_t)b * a.H + iy) * a.W + ix) * a.ldy + ch * 4) =
                    *reinterpret_cast<const float4*>(stg + row * X3_FP + ch * 16);
            }
          }
        }
      }
    }
    if (a.stats != nullptr) {
      float* sred = reinterpret_cast<float*>(smem + X3_SRED_OFF);   // [wave][64][2]
      float* scnt = sred + 4 * 64 * 2;
      int cnt = __builtin_popcount(vmask[0]) + __builtin_popcount(vmask[1]);
      cnt += __shfl_xor(cnt, 32);
      const float inv = 1.f / (float)(cnt > 0 ? cnt : 1);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float sm = 0.f, q = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) sm += ((vmask[i] >> r) & 1u) ? acc[i][j][r] : 0.f;
        sm += __shfl_xor(sm, 32);
        const float mean = sm * inv;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float d = acc[i][j][r] - mean;
            q += ((vmask[i] >> r) & 1u) ? d * d : 0.f;
          }
        q += __shfl_xor(q, 32);
        if (h == 0) {
          sred[(wave * 64 + j * 32 + l31) * 2 + 0] = sm;
          sred[(wave * 64 + j * 32 + l31) * 2 + 1] = q;
        }
      }
      if (lane == 0) scnt[wave] = (float)cnt;
      __syncthreads();
      if (threadIdx.x < 64) {
        const int col = threadIdx.x;
        double n_tot = 0.0, s_tot = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { n_tot += (double)scnt[k]; s_tot += (double)sred[(k * 64 + col) * 2]; }
        const double mu = n_tot > 0.0 ? s_tot / n_tot : 0.0;
        double m2 = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double nk = (double)scnt[k];
          if (nk > 0.0) {
            const double d = (double)sred[(k * 64 + col) * 2] / nk - mu;
            m2 += (double)sred[(k * 64 + col) * 2 + 1] + nk * d * d;
          }
        }
        a.stats[((int64_t)tile * 2 + 0) * 64 + col] = (float)s_tot;
        a.stats[((int64_t)tile * 2 + 1) * 64 + col] = (float)m2;
        if (col == 0) a.stats[(int64_t)a.ntiles * 2 * 64 + tile] = (float)n_tot;
      }
    }
  }
}

// ---- pipelined tile loop (SFOD_F1_PIPE=1, the default) --------------------------------------------------------------------
// Same tiles, same MFMA order per accumulator, same epilogue arithmetic as f1_x3_plain -- every output is bit-identical --
// with the work around the MFMAs cut down:
//   * tile n + 1's patch is in flight (3 x 16 bytes per thread, in registers) while tile n computes and stores; it goes to
//     LDS at the top of the next iteration.  One barrier (patch written -> fragments read) instead of two; the second one a
//     single patch buffer needs (fragments read -> patch rewritten) is the one the statistics have anyway.  The
//     statistics-only pass stages no output, keeps two patch buffers and has ONE barrier per tile.
//   * a thread's chunk -> (py, px, half) decode and its fragment offsets are computed once per workgroup; the tile
//     coordinates advance by the grid stride with carries: no division in the loop.
//   * a weight fragment is read once per (k-step, j) and used for both pixel rows.
//   * full tiles (workgroup-uniform) run without row masks, in the statistics and at the stores.
//   * the fp64 combine of tile n's partial statistics runs after tile n + 1's barrier (two partial buffers), beside the
//     other waves' MFMAs, on a wave that rotates with the tile; on a full tile its divisions are by 64 and 256.
// From here to the end of the file every rounding is written out (what the compiler made of f1_x3_plain's expressions:
// contraction depends on the surroundings).
#pragma clang fp contract(off)

// (sum, M2, count) of the four waves -> statistics block `tile`; one thread per column.  On a full tile every count is
// 64: the five fp64 divisions are by 64 and 256, i.e. exact, and so are the multiplications that stand for them.
__device__ __forceinline__ void f1_combine(const F1Args& a, const float* sred, int tile, int col, bool full) {
  const float* scnt = sred + 4 * 64 * 2;
  double n_tot = 0.0, s_tot = 0.0, m2 = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) s_tot += (double)sred[(k * 64 + col) * 2];
  if (full) {
    n_tot = 256.0;
    const double mu = s_tot * (1.0 / 256.0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double d = (double)sred[(k * 64 + col) * 2] * (1.0 / 64.0) - mu;
      m2 += __builtin_fma(d, 64.0 * d, (double)sred[(k * 64 + col) * 2 + 1]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) n_tot += (double)scnt[k];
    const double mu = n_tot > 0.0 ? s_tot / n_tot : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double nk = (double)scnt[k];
      if (nk > 0.0) {
        const double d = (double)sred[(k * 64 + col) * 2] / nk - mu;
        m2 += __builtin_fma(d, nk * d, (double)sred[(k * 64 + col) * 2 + 1]);
      }
    }
  }
  a.stats[((int64_t)tile * 2 + 0) * 64 + col] = (float)s_tot;
  a.stats[((int64_t)tile * 2 + 1) * 64 + col] = (float)m2;
  if (col == 0) a.stats[(int64_t)a.ntiles * 2 * 64 + tile] = (float)n_tot;
}

template <int FMT, int MODE>
__device__ __forceinline__ void f1_x3_pipe(const F1Args& a, unsigned char* smem) {
  using pair_t = typename std::conditional<FMT == 2, splith_t, split_t>::type;
  constexpr bool DB = (MODE == F1_STATS);      // two patch buffers
  const bool with_stats = MODE != F1_BN && a.stats != nullptr;      // (F1_BN follows a pass that made them)
  const float winv = (FMT == 2 && a.wamax != nullptr) ? winv_from_absmax(*a.wamax) : 1.0f;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int G = gridDim.x;
  int tile = blockIdx.x;
  if (tile >= a.ntiles) return;
  for (int e = tid; e < 5 * 2 * 64; e += 256) {
    const int ln = e & 63, j = (e >> 6) & 1, ks = e >> 7;
    const int tap = 2 * ks + (ln >> 5);
    uint4 vh = make_uint4(0, 0, 0, 0), vl = vh;
    if (tap < 9) {
      const uint4* p = reinterpret_cast<const uint4*>(a.w + ((j * 32 + (ln & 31)) * 9 + tap) * 16);
      vh = p[0];
      vl = p[1];
    }
    *reinterpret_cast<uint4*>(smem + X3_W_OFF + (((ks * 2 + j) * 2 + 0) * 64 + ln) * 16) = vh;
    *reinterpret_cast<uint4*>(smem + X3_W_OFF + (((ks * 2 + j) * 2 + 1) * 64 + ln) * 16) = vl;
  }
  // per-column constants.  F1_AFFINE: c0 = scale, c1 = shift.  F1_BN: c0 = mean, c1 = invstd * gamma, c2 = beta
  float bcol[2], c0[2], c1[2], c2[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = j * 32 + l31;
    bcol[j] = a.bias ? a.bias[c] : 0.f;
    c0[j] = c1[j] = c2[j] = 0.f;
    if constexpr (MODE == F1_AFFINE) { c0[j] = a.scale[c]; c1[j] = a.shift[c]; }
    if constexpr (MODE == F1_BN) { c0[j] = a.mean[c]; c1[j] = a.invstd[c] * a.gamma[c]; c2[j] = a.beta[c]; }
  }
  const float lo = (a.act == 1) ? 0.f : -__builtin_inff();

  // tile-invariant: this thread's patch chunks (tid + 256 k; the third one exists for tid < 168) ...
  int cpyx[3], crel[3];      // (py << 8 | px) and the chunk's byte offset from the patch origin (sfod_f1_launch: fits an int)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int p = tid + 256 * k, pp = p >> 1, half = p & 1;
    const int py = pp / PW, px = pp - py * PW;
    cpyx[k] = (py << 8) | px;
    crel[k] = (py * a.W + px) * 32 + half * 16;
  }
  const bool third = tid < PH * PW * 2 - 512;
  // ... and its A-fragment offsets: k-step s reads patch pixel (2 wave + i + ky, l31 + kx) of tap 2 s + h
  int aoff[5];
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const int tap = 2 * s + h;
    const int ky = tap / 3, kx = tap - ky * 3;
    aoff[s] = ((2 * wave + ky) * PW + l31 + kx) * 32;
  }
  // the grid stride in tile coordinates
  const int tyx = a.tiles_y * a.tiles_x;
  const int sb = G / tyx, sy = (G - sb * tyx) / a.tiles_x, sx = G - sb * tyx - sy * a.tiles_x;
  int b = tile / tyx, tyi = (tile - b * tyx) / a.tiles_x, txi = tile - b * tyx - tyi * a.tiles_x;

  uint4 pre[3];
  auto fetch = [&](int fb, int fty, int ftx) {
    const int ym = fty * TH - 1, xm = ftx * TW - 1;
    const int64_t base = (((int64_t)fb * a.H + ym) * a.W + xm) * 32;      // bytes; before the buffer for the first tile
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int iy = ym + (cpyx[k] >> 8), ix = xm + (cpyx[k] & 255);
      const bool ok = (k < 2 || third) && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      // an out-of-image chunk reads the buffer's first 16 bytes and becomes zeros
      const uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(a.x) + (ok ? base + crel[k] : 0));
      pre[k] = ok ? v : make_uint4(0, 0, 0, 0);
    }
  };
  fetch(b, tyi, txi);

  float* const sred0 = reinterpret_cast<float*>(smem + X3_SRED_OFF);      // [2][ [wave][64][2] + [4] ]
  int prev_tile = -1, it = 0;
  bool prev_full = false;
  for (;; ++it) {
    const int x0 = txi * TW, y0 = tyi * TH;
    unsigned char* patch = smem + ((DB && (it & 1)) ? X3_STG_OFF : 0);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < 2 || third) *reinterpret_cast<uint4*>(patch + (tid + 256 * k) * 16) = pre[k];
    // the next tile of this workgroup
    const int ntile = tile + G;
    const bool more = ntile < a.ntiles;
    int nb = b + sb, nty = tyi + sy, ntx = txi + sx;
    if (ntx >= a.tiles_x) { ntx -= a.tiles_x; ++nty; }
    if (nty >= a.tiles_y) { nty -= a.tiles_y; ++nb; }
    if (more) fetch(nb, nty, ntx);
    __syncthreads();      // patch written; everybody is past the previous tile's fragment reads and partial statistics
    // (the combining wave rotates: with three workgroups per CU the fp64 work spreads over the four SIMDs)
    if (with_stats && prev_tile >= 0 && wave == ((it - 1) & 3))
      f1_combine(a, sred0 + ((it - 1) & 1) * (X3_SRED_BYTES / 4), prev_tile, lane, prev_full);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        uint4 vh = make_uint4(0, 0, 0, 0), vl = vh;
        if (s < 4 || h == 0) {      // tap 9 is padding
          vh = *reinterpret_cast<const uint4*>(patch + aoff[s] + i * (PW * 32));
          vl = *reinterpret_cast<const uint4*>(patch + aoff[s] + i * (PW * 32) + 16);
        }
        ah[i] = __builtin_bit_cast(bf16x8, vh);
        al[i] = __builtin_bit_cast(bf16x8, vl);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bh[j] = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const uint4*>(smem + X3_W_OFF + (((s * 2 + j) * 2 + 0) * 64 + lane) * 16));
        bl[j] = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const uint4*>(smem + X3_W_OFF + (((s * 2 + j) * 2 + 1) * 64 + lane) * 16));
      }
      // per accumulator: ah * bl, al * bh, ah * bh of k-step s, as in f1_x3_plain; four independent chains interleaved
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma_pairs<FMT>(ah[i], bl[j], acc[i][j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma_pairs<FMT>(al[i], bh[j], acc[i][j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma_pairs<FMT>(ah[i], bh[j], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          acc[i][j][r] = (FMT == 2) ? __builtin_fmaf(acc[i][j][r], winv, bcol[j]) : acc[i][j][r] + bcol[j];

    const bool full = (y0 + TH <= a.H) && (x0 + TW <= a.W);      // workgroup-uniform
    // one tile's stores and partial statistics; FULL: no row masks, no bounds tests
    auto epilogue = [&](auto full_c) {
      constexpr bool FULL = decltype(full_c)::value;
      unsigned vmask[2] = {0xffffu, 0xffffu};
      if constexpr (!FULL) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          unsigned m = 0;
          const int iy = y0 + 2 * wave + i;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int px = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (iy < a.H && x0 + px < a.W) m |= (1u << r);
          }
          vmask[i] = m;
        }
      }
      if constexpr (MODE != F1_STATS) {
        unsigned char* stg = smem + X3_STG_OFF + wave * (16 * X3_FP);
#pragma unroll
        for (int i = 0; i < 2; ++i) {          // M-fragment i = the 32 pixels of image row y0 + 2 * wave + i
          const int iy = y0 + 2 * wave + i;
#pragma unroll
          for (int qh = 0; qh < 2; ++qh) {     // pixels 16 * qh .. 16 * qh + 15 (accumulator registers 8 * qh .. 8 * qh + 7)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int rr = 0; rr < 8; ++rr) {
                const int r = qh * 8 + rr;
                const int ml = (rr & 3) + 8 * (rr >> 2) + 4 * h;
                float o;
                if constexpr (MODE == F1_AFFINE) {
                  o = fmaxf(__builtin_fmaf(acc[i][j][r], c0[j], c1[j]), lo);
                } else if constexpr (MODE == F1_BN) {
                  // y as pass 1 stored it, then k_bn_relu_pool_fwd's expression: fma(y - mean, invstd * gamma, beta), ReLU
                  const float yv = fmaxf(__builtin_fmaf(acc[i][j][r], 1.f, 0.f), -__builtin_inff());
                  o = fmaxf(__builtin_fmaf(yv - c0[j], c1[j], c2[j]), 0.f);
                } else {
                  o = fmaxf(__builtin_fmaf(acc[i][j][r], 1.f, 0.f), lo);
                }
                *reinterpret_cast<float*>(stg + ml * X3_FP + (j * 32 + l31) * 4) = o;
              }
            if constexpr (MODE == F1_AFFINE || MODE == F1_BN) {
              // 8 lanes per pixel: 8 consecutive channels -> one 32-byte (hi | lo) group
#pragma unroll
              for (int it2 = 0; it2 < 2; ++it2) {
                const int row = it2 * 8 + (lane >> 3), gch = lane & 7;
                const int ix = x0 + qh * 16 + row;
                if (FULL || (iy < a.H && ix < a.W)) {
                  const float4 v0 = *reinterpret_cast<const float4*>(stg + row * X3_FP + gch * 32);
                  const float4 v1 = *reinterpret_cast<const float4*>(stg + row * X3_FP + gch * 32 + 16);
                  const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                  split_store8(reinterpret_cast<pair_t*>(a.y) + (((int64_t)b * a.H + iy) * a.W + ix) * a.ldy + gch * 8, f);
                }
              }
            } else {
#pragma unroll
              for (int it2 = 0; it2 < 4; ++it2) {
                const int row = it2 * 4 + (lane >> 4), ch = lane & 15;
                const int ix = x0 + qh * 16 + row;
                if (FULL || (iy < a.H && ix < a.W))
                  *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.y) + (((int64_t)b * a.H + iy) * a.W + ix) * a.ldy + ch * 4) =
                      *reinterpret_cast<const float4*>(stg + row * X3_FP + ch * 16);
              }
            }
          }
        }
      }
      if (with_stats) {
        float* sred = sred0 + (it & 1) * (X3_SRED_BYTES / 4);   // [wave][64][2]
        float* scnt = sred + 4 * 64 * 2;
        int cnt = 64;
        if constexpr (!FULL) {
          cnt = __builtin_popcount(vmask[0]) + __builtin_popcount(vmask[1]);
          cnt += __shfl_xor(cnt, 32);
        }
        const float inv = 1.f / (float)(cnt > 0 ? cnt : 1);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float sm = 0.f, q = 0.f;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) sm = sm + ((FULL || ((vmask[i] >> r) & 1u)) ? acc[i][j][r] : 0.f);
          sm = sm + __shfl_xor(sm, 32);
          // (the mean is never rounded on its own: v - sm * inv is one fused operation)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float d = __builtin_fmaf(-inv, sm, acc[i][j][r]);
              const float dd = d * d;
              q = q + ((FULL || ((vmask[i] >> r) & 1u)) ? dd : 0.f);
            }
          q = q + __shfl_xor(q, 32);
          if (h == 0) {
            sred[(wave * 64 + j * 32 + l31) * 2 + 0] = sm;
            sred[(wave * 64 + j * 32 + l31) * 2 + 1] = q;
          }
        }
        if (lane == 0) scnt[wave] = (float)cnt;
      }
    };
    if (full) epilogue(std::true_type{});
    else epilogue(std::false_type{});

    if (!DB) __syncthreads();      // the one patch buffer is rewritten next: everybody's fragment reads are done
    prev_full = full;
    if (!more) break;
    prev_tile = tile;
    tile = ntile;
    b = nb; tyi = nty; txi = ntx;
  }
  if (with_stats) {
    if (DB) __syncthreads();
    if (wave == (it & 3)) f1_combine(a, sred0 + (it & 1) * (X3_SRED_BYTES / 4), tile, lane, prev_full);      // the last tile's
  }
}

template <int FMT, int MODE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_conv_first_x3(F1Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[MODE == F1_PLAIN ? X3_LDS_BYTES : X3_PIPE_LDS_BYTES];
  if constexpr (MODE == F1_PLAIN) f1_x3_plain<FMT>(a, smem);
  else f1_x3_pipe<FMT, MODE>(a, smem);
}

}  // namespace

constexpr int F1_PIPE_MAX_W = 1 << 22;
bool sfod_f1_bn_ok(int W) { return W <= F1_PIPE_MAX_W; }

int sfod_f1_nblk(int B, int H, int W) { return B * ((H + TH - 1) / TH) * ((W + TW - 1) / TW); }

// A/B knobs.  SFOD_F1_PIPE: 1 (default) the pipelined tile loop of the bf16x3 / f16x3 kernel, 0 the plain one -- same bits.
// SFOD_F1_GRID: 0 (default) the persistent grid is one workgroup per resident slot (768 for the pair formats, 2048 for
// bf16); n > 0 caps it at n workgroups (tests: several tiles per workgroup on small images).
static SfodKnob g_f1_pipe{"SFOD_F1_PIPE", 1, sfod_knob_bool};
static SfodKnob g_f1_grid{"SFOD_F1_GRID", 0, [](int n) { return n > 0 ? n : 0; }};
extern "C" int sfod_set_conv_first_pipe(int on) { g_f1_pipe.set(on); return 0; }
extern "C" int sfod_set_conv_first_grid(int n) { g_f1_grid.set(n); return 0; }

template <int FMT>
static void f1_x3_dispatch(int mode, int grid, hipStream_t s, const F1Args& a) {
  switch (mode) {
    case F1_STATS: hipLaunchKernelGGL((k_conv_first_x3<FMT, F1_STATS>), dim3(grid), dim3(256), 0, s, a); break;
    case F1_Y: hipLaunchKernelGGL((k_conv_first_x3<FMT, F1_Y>), dim3(grid), dim3(256), 0, s, a); break;
    case F1_AFFINE: hipLaunchKernelGGL((k_conv_first_x3<FMT, F1_AFFINE>), dim3(grid), dim3(256), 0, s, a); break;
    case F1_BN:      // bf16 pairs only (sfod_f1_launch)
      if constexpr (FMT == 1) hipLaunchKernelGGL((k_conv_first_x3<FMT, F1_BN>), dim3(grid), dim3(256), 0, s, a);
      break;
    default: hipLaunchKernelGGL((k_conv_first_x3<FMT, F1_PLAIN>), dim3(grid), dim3(256), 0, s, a); break;
  }
}

// split 1 / 2: SFOD_BF16X3 / SFOD_F16X3 operands; y is fp32 (scale == nullptr) or operand pairs (scale / shift given)
int sfod_f1_launch(const void* x, const void* w, const float* bias, void* y, float* stats, int B, int H, int W,
                   int ldy, int act, hipStream_t s, const float* scale, const float* shift, int split, const unsigned* wamax,
                   const F1BnApply* bn) {
  F1Args a;
  a.wamax = wamax;
  a.x = (const bf16_t*)x; a.w = (const bf16_t*)w; a.bias = bias; a.y = y; a.stats = stats;
  a.scale = scale; a.shift = shift;
  a.mean = bn ? bn->mean : nullptr; a.invstd = bn ? bn->invstd : nullptr;
  a.gamma = bn ? bn->gamma : nullptr; a.beta = bn ? bn->beta : nullptr;
  a.B = B; a.H = H; a.W = W; a.ldy = ldy; a.act = act;
  a.tiles_y = (H + TH - 1) / TH; a.tiles_x = (W + TW - 1) / TW;
  a.ntiles = B * a.tiles_y * a.tiles_x;
  if (a.ntiles == 0) return 0;  const int resident = split ? 256 * 3 : 256 * 8;      // bf16x3: 3 workgroups per CU (LDS), each stages the weights once
  int grid = a.ntiles < resident ? a.ntiles : resident;
  const int cap = g_f1_grid.get();
  if (cap > 0 && grid > cap) grid = cap;
  sfod_note_conv_kernel(split == 2 ? "k_conv_first_x3<2>" : (split ? "k_conv_first_x3<1>" : "k_conv_first"));
  if (split) {
    // the BatchNorm epilogue exists in the pipelined loop only (it is one of its instantiations)
    const bool pipe_ok = W <= F1_PIPE_MAX_W;      // its patch offsets are 32-bit
    SFOD_REQUIRE(bn == nullptr || (y != nullptr && scale == nullptr && split == 1 && pipe_ok),
                 "conv_first: BatchNorm epilogue on bf16 pairs");
    const int mode = bn ? F1_BN : (!(g_f1_pipe.get() && pipe_ok) ? F1_PLAIN : (y == nullptr ? F1_STATS : (scale ? F1_AFFINE : F1_Y)));
    if (split == 2) f1_x3_dispatch<2>(mode, grid, s, a);
    else f1_x3_dispatch<1>(mode, grid, s, a);
  } else {
    SFOD_REQUIRE(bn == nullptr, "conv_first: BatchNorm epilogue on bf16 pairs");
    hipLaunchKernelGGL(k_conv_first, dim3(grid), dim3(256), 0, s, a);
  }
  return sfod_check_launch("conv_first");
}

SFOD_DEFINE_F16_POLL(sfod_f16_poll_first)
