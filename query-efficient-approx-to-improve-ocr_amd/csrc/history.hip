// Label-history loss weights: the [n][W+1] table of one minibatch in one launch (include/qea_hip.h: qea_history_lev_weights,
// qea_history_attn_weights).  Limits: W <= QEA_HISTORY_MAX_WINDOW (8), words of <= QEA_HISTORY_MAX_LEN (128) code points for the
// Levenshtein table, (V1 + W) * Dq <= QEA_HISTORY_ATTN_MAX_TABLE floats for the attention table.
//
// history_lev_kernel: one wave per workgroup, one LANE per unordered pair of words (W(W-1)/2 pairs per strip, S = LEV_LANES / pairs
// strips per workgroup, capped so that the staged characters fit).  The characters of the workgroup's words sit in LDS
// character-major (tok[c * slots + word]: the lanes of a pair loop read the same c, so at most the words differ), the DP row of a
// lane column-major (row[j * 64 + lane]: conflict-free); the recursion is edit_distance.h's, the one edit_distance_kernel runs.
// The distances meet in LDS; one lane per (strip, word) sums them as integers and evaluates the weight in fp64 with every operation
// rounded separately, as CPython does.
//
// history_attn_kernel: Wq is linear, so  q[w] = (1/n_chars) sum_c T[idx[w][c]] + P[w]  with  T = embedding Wq^T  [V1][Dq]  and
// P = positional_encodings Wq^T + bias  [W][Dq].  Every workgroup builds T and P once in LDS ((V1 + W) * Dq floats, 12.6 KB at the
// default sizes; 0.8 MFLOP) and then walks strips, one WAVE per strip: the gather-sum of T rows (four partial sums per element),
// then lane i owns row i of softmax(q q^T / sqrt(Dq)), its Linear(W -> 1) and the activation.  fp32 throughout, no MFMA.
#include "common.h"
#include "edit_distance.h"
#include <math.h>

namespace {

constexpr int HW_MAX = QEA_HISTORY_MAX_WINDOW;
constexpr int LEV_L = ED_MAX;
constexpr int LEV_LANES = ED_LANES;
constexpr int LEV_SLOTS = 56;                       // words staged per workgroup: 56 * 128 * 4 B = 28 KB next to the 33 KB of DP rows
constexpr int ATTN_THREADS = 256;
constexpr int ATTN_WAVES = ATTN_THREADS / QEA_WAVE;

// strips per workgroup at window W (host and device agree on it)
__host__ __device__ constexpr int lev_strips(int W) {
  const int pairs = W * (W - 1) / 2;
  const int by_lanes = pairs > 0 ? LEV_LANES / pairs : LEV_LANES;
  const int by_slots = LEV_SLOTS / W;
  return by_lanes < by_slots ? by_lanes : by_slots;
}

__global__ __launch_bounds__(LEV_LANES) void history_lev_kernel(const int* __restrict__ tokens, const int* __restrict__ lens,
                                                                const int* __restrict__ count, int n, int W, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ int row[(LEV_L + 1) * LEV_LANES];
  __shared__ int tok[LEV_L * LEV_SLOTS];
  __shared__ int wlen[LEV_SLOTS];
  __shared__ int dist[LEV_SLOTS * HW_MAX];            // dist[(s * W + a) * W + b], both orders
  const int lane = threadIdx.x;
  const int S = lev_strips(W), pairs = W * (W - 1) / 2, slots = S * W;
  const int r0 = blockIdx.x * S;                      // first strip of this workgroup
  // stage lengths, then characters (c fastest in global memory, word fastest in LDS)
  if (lane < slots) {
    const int r = r0 + lane / W;
    wlen[lane] = r < n ? min(max(lens[(size_t)r * W + lane % W], 0), LEV_L) : 0;
  }
  __syncthreads();
  for (int sl = 0; sl < slots; ++sl) {
    const int r = r0 + sl / W;
    if (r >= n) break;                                // uniform: sl does not depend on the lane
    const int* src = tokens + ((size_t)r * W + sl % W) * LEV_L;
    const int len = wlen[sl];
    for (int c = lane; c < len; c += LEV_LANES) tok[c * slots + sl] = src[c];
  }
  __syncthreads();
  // one pair per lane
  const int s = pairs > 0 ? lane / pairs : S;         // local strip of this lane (S: no pair)
  if (s < S && r0 + s < n) {
    int p = lane - s * pairs, a = 0;
    while (p >= W - 1 - a) {                          // pairs in order (0,1) (0,2) .. (0,W-1) (1,2) ..
      p -= W - 1 - a;
      ++a;
    }
    const int b = a + 1 + p;
    const int cnt = min(max(count[r0 + s], 0), W);
    if (b < cnt) {
      const int sa = s * W + a, sb = s * W + b;
      const int d = edit_distance_lane(row, lane, wlen[sa], wlen[sb], [&](int i) { return tok[i * slots + sa]; },
                                       [&](int j) { return tok[j * slots + sb]; });
      dist[sa * W + b] = d;
      dist[sb * W + a] = d;
    }
  }
  __syncthreads();
  // one (strip, word) per lane: integer sum, fp64 epilogue, one rounding to fp32
  if (lane < slots) {
    const int sl = lane / W, i = lane % W, r = r0 + sl;
    if (r < n) {
      const int cnt = min(max(count[r], 0), W);
      float* o = out + (size_t)r * (W + 1);
      if (i == 0) o[0] = 1.f;
      float v = 0.f;
      if (i < cnt) {
        int sum = 0;
        for (int j = 0; j < cnt; ++j)
          if (j != i) sum += dist[lane * W + j];
        const double others = (double)max(cnt - 1, 1);
        const double mean = (double)sum / others;
        const double chars = (double)max(1, wlen[lane]);
        const double q = fmin(mean, chars) / chars;
        const double one_minus = 1.0 - q;
        v = (float)(0.5 * one_minus);
      }
      o[i + 1] = v;
    }
  }
}

// dot of two 16-byte aligned fp32 rows of length E (a multiple of 4), four partial sums
__device__ __forceinline__ float attn_dot(const float* __restrict__ a, const float* __restrict__ b, int E) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int e = 0; e < E; e += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(a + e);
    const f32x4 y = *reinterpret_cast<const f32x4*>(b + e);
    acc += x * y;
  }
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

__global__ __launch_bounds__(ATTN_THREADS) void history_attn_kernel(const int* __restrict__ char_idx, const int* __restrict__ count, int n,
                                                                    int W, int n_chars, const float* __restrict__ emb, int V1, int E,
                                                                    const float* __restrict__ wq_w, const float* __restrict__ wq_b, int Dq,
                                                                    const float* __restrict__ coef_w, const float* __restrict__ coef_b,
                                                                    const float* __restrict__ pos, int activation, float* __restrict__ out) {
  extern __shared__ float attn_smem[];
  float* T = attn_smem;                               // [V1 + W][Dq]: rows V1.. are P
  __shared__ float zs[ATTN_WAVES][HW_MAX];
  float* q_all = T + (size_t)(V1 + W) * Dq;           // [ATTN_WAVES][W][Dq + 1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int o = tid; o < (V1 + W) * Dq; o += ATTN_THREADS) {
    const int v = o / Dq, d = o - v * Dq;
    const float* src = v < V1 ? emb + (size_t)v * E : pos + (size_t)(v - V1) * E;
    const float t = attn_dot(src, wq_w + (size_t)d * E, E);
    T[o] = v < V1 ? t : t + wq_b[d];
  }
  __syncthreads();
  const float* P = T + (size_t)V1 * Dq;
  float* q = q_all + (size_t)wave * W * (Dq + 1);
  const float inv_chars = 1.f / (float)n_chars, inv_sqrt = 1.f / sqrtf((float)Dq);
  const float cb = coef_b[0];
  for (int base = blockIdx.x * ATTN_WAVES; base < n; base += gridDim.x * ATTN_WAVES) {     // uniform over the workgroup
    const int r = base + wave;
    const int cnt = r < n ? min(max(count[r], 0), W) : 0;
    if (cnt > 0) {
      const int* idx = char_idx + (size_t)r * W * n_chars;
      for (int e = lane; e < W * Dq; e += QEA_WAVE) {
        const int w = e / Dq, d = e - w * Dq;
        const int* iw = idx + w * n_chars;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int c = 0;
        for (; c + 4 <= n_chars; c += 4) {
          a0 += T[min(max(iw[c], 0), V1 - 1) * Dq + d];
          a1 += T[min(max(iw[c + 1], 0), V1 - 1) * Dq + d];
          a2 += T[min(max(iw[c + 2], 0), V1 - 1) * Dq + d];
          a3 += T[min(max(iw[c + 3], 0), V1 - 1) * Dq + d];
        }
        for (; c < n_chars; ++c) a0 += T[min(max(iw[c], 0), V1 - 1) * Dq + d];
        q[w * (Dq + 1) + d] = ((a0 + a1) + (a2 + a3)) * inv_chars + P[e];
      }
    }
    __syncthreads();
    if (cnt > 0 && lane < W) {
      float sc[HW_MAX];
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < HW_MAX; ++j) {
        sc[j] = 0.f;
        if (j < W) {
          float acc = 0.f;
          for (int d = 0; d < Dq; ++d) acc += q[lane * (Dq + 1) + d] * q[j * (Dq + 1) + d];
          sc[j] = acc * inv_sqrt;
          m = fmaxf(m, sc[j]);
        }
      }
      float den = 0.f;
#pragma unroll
      for (int j = 0; j < HW_MAX; ++j)
        if (j < W) {
          sc[j] = expf(sc[j] - m);
          den += sc[j];
        }
      float z = 0.f;
#pragma unroll
      for (int j = 0; j < HW_MAX; ++j)
        if (j < W) z += (sc[j] / den) * coef_w[j];
      zs[wave][lane] = z + cb;
    }
    __syncthreads();
    if (r < n && lane <= W) {
      float v = lane == 0 ? 1.f : 0.f;
      if (lane > 0 && lane - 1 < cnt) {
        const float z = zs[wave][lane - 1];
        if (activation == QEA_HISTORY_ACT_SIGMOID) {
          v = 1.f / (1.f + expf(-z));
        } else if (activation == QEA_HISTORY_ACT_SOFTMAX) {
          float m = -INFINITY, den = 0.f;
          for (int j = 0; j < W; ++j) m = fmaxf(m, zs[wave][j]);
          for (int j = 0; j < W; ++j) den += expf(zs[wave][j] - m);
          v = expf(z - m) / den;
        } else {
          float sum = 0.f;
          for (int j = 0; j < W; ++j) sum += fmaxf(zs[wave][j], 0.f);
          v = fmaxf(z, 0.f) / (sum + 0.000001f);
        }
      }
      out[(size_t)r * (W + 1) + lane] = v;
    }
    __syncthreads();                                  // the next round overwrites q and zs
  }
}

}  // namespace

extern "C" int qea_history_lev_weights(const int32_t* tokens, const int32_t* lens, const int32_t* count, int32_t n, int32_t W, float* out,
                                       void* stream) {
  QEA_REQUIRE(tokens && lens && count && out, "qea_history_lev_weights: null pointer");
  QEA_REQUIRE(n >= 1 && n <= (1 << 24), "qea_history_lev_weights: n=%d outside 1..2^24", n);
  QEA_REQUIRE(W >= 1 && W <= HW_MAX, "qea_history_lev_weights: window %d outside 1..%d", W, HW_MAX);
  hipLaunchKernelGGL(history_lev_kernel, dim3(qea_cdiv(n, lev_strips(W))), dim3(LEV_LANES), 0, (hipStream_t)stream, tokens, lens, count, n, W,
                     out);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_history_attn_weights(const int32_t* char_idx, const int32_t* count, int32_t n, int32_t W, int32_t n_chars,
                                        const float* embedding, int32_t V1, int32_t E, const float* wq_weight, const float* wq_bias,
                                        int32_t Dq, const float* coef_weight, const float* coef_bias, const float* positional_encodings,
                                        int32_t activation, float* out, void* stream) {
  QEA_REQUIRE(char_idx && count && embedding && wq_weight && wq_bias && coef_weight && coef_bias && positional_encodings && out,
              "qea_history_attn_weights: null pointer");
  QEA_REQUIRE(n >= 1 && n <= (1 << 24), "qea_history_attn_weights: n=%d outside 1..2^24", n);
  QEA_REQUIRE(W >= 1 && W <= HW_MAX, "qea_history_attn_weights: window %d outside 1..%d", W, HW_MAX);
  QEA_REQUIRE(n_chars >= 1 && n_chars <= 4096, "qea_history_attn_weights: n_chars=%d outside 1..4096", n_chars);
  QEA_REQUIRE(V1 >= 1 && Dq >= 1 && (long long)(V1 + W) * Dq <= QEA_HISTORY_ATTN_MAX_TABLE,
              "qea_history_attn_weights: (V1 + W) * Dq = (%d + %d) * %d exceeds %d", V1, W, Dq, QEA_HISTORY_ATTN_MAX_TABLE);
  QEA_REQUIRE(E >= 4 && E % 4 == 0 && E <= (1 << 16), "qea_history_attn_weights: E=%d must be a multiple of 4 in 4..65536", E);
  QEA_REQUIRE((((uintptr_t)embedding | (uintptr_t)wq_weight | (uintptr_t)positional_encodings) & 15) == 0,
              "qea_history_attn_weights: embedding, wq_weight and positional_encodings must be 16-byte aligned");
  QEA_REQUIRE(activation >= QEA_HISTORY_ACT_SIGMOID && activation <= QEA_HISTORY_ACT_RELU, "qea_history_attn_weights: unknown activation %d",
              activation);
  // enough workgroups to fill the device, few enough that the per-workgroup table (0.8 MFLOP) stays a small share of the work
  const int grid = min(qea_cdiv(n, ATTN_WAVES * 2), 256);
  const size_t lds = ((size_t)(V1 + W) * Dq + (size_t)ATTN_WAVES * W * (Dq + 1)) * sizeof(float);
  hipLaunchKernelGGL(history_attn_kernel, dim3(grid), dim3(ATTN_THREADS), lds, (hipStream_t)stream, char_idx, count, n, W, n_chars, embedding,
                     V1, E, wq_weight, wq_bias, Dq, coef_weight, coef_bias, positional_encodings, activation, out);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
