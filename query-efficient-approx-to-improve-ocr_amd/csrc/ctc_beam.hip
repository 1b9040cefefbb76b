// CTC prefix beam search (include/qea_hip.h: qea_ctc_beam_decode; the specification is DESIGN.md "CTC prefix beam search").
// The reference decodes greedily only (utils.py:74-92); this is the decoder that adds up the alignments of a labelling.
//
// ONE 256-thread workgroup per sample, no communication between workgroups, no atomics, no workspace; every output element is
// stored once.  All scores are fp64: a step needs O(K) log1p/exp (the stay slots and the folded merges), the K * C extension
// scores are one add each.
//
// LDS: two generations of the beam's prefixes as bytes (dynamic, 2 * K * T <= 32 KB), per entry its length, last token, rolling
// 64-bit hash and its parent's hash, pb / pnb / tot; the current row of log-probs as fp64 (2 KB); a K x C byte table of the
// extension slots that were folded into another entry's stay slot (8 KB).
// Candidate (owner rank i, slot s) has index i * C + s, thread (index & 255) keeps it in register (index >> 8): ascending index is
// the specification's candidate order, so "largest score, lowest index" K times is the stable descending sort.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int BEAM_THREADS = 256;
constexpr int BEAM_MAX_K = 32, BEAM_MAX_C = 256, BEAM_MAX_T = 512;
constexpr unsigned long long BEAM_HASH_SEED = 0x9E3779B97F4A7C15ull, BEAM_HASH_MUL = 0x100000001B3ull;

__device__ __forceinline__ double beam_lse(double a, double b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  return fmax(a, b) + log1p(exp(-fabs(a - b)));
}

// (score, index) ordering of the selection: the larger score, on equal scores the lower candidate index
__device__ __forceinline__ bool beam_before(double s, int i, double s2, int i2) { return s > s2 || (s == s2 && i < i2); }

// slot s >= 1 of a beam entry is the s-th class that is not the blank, ascending
__device__ __forceinline__ int beam_slot_class(int s, int blank) { return s <= blank ? s - 1 : s; }

// R: candidate registers per thread, K * C <= R * 256
template <int R>
__global__ __launch_bounds__(BEAM_THREADS) void ctc_beam_kernel(const float* __restrict__ scores, int ld_t, int ld_n, int T, int C, int blank,
                                                                 int K, int* __restrict__ tokens, int* __restrict__ lengths,
                                                                 double* __restrict__ beam_scores) {
  extern __shared__ __align__(16) unsigned char pre[];                 // [2][K][T] prefixes, one byte per token
  __shared__ double row[BEAM_MAX_C];                                    // lp[t][:] as fp64, NaN -> -inf
  __shared__ double s_pb[2][BEAM_MAX_K], s_pnb[2][BEAM_MAX_K], s_tot[2][BEAM_MAX_K];
  __shared__ unsigned long long s_hash[2][BEAM_MAX_K], s_phash[2][BEAM_MAX_K];
  __shared__ int s_len[2][BEAM_MAX_K], s_last[2][BEAM_MAX_K];
  __shared__ double stay_pb[BEAM_MAX_K], stay_pnb[BEAM_MAX_K];        // slot 0 of every entry, merges folded in
  __shared__ int parent[BEAM_MAX_K];                                    // rank of the entry whose prefix + last token is entry j, or -1
  __shared__ unsigned char folded[BEAM_MAX_K * BEAM_MAX_C];             // [i][c] != 0: slot of class c of entry i does not exist
  __shared__ double red_s[2][BEAM_THREADS / 64], sel_s[BEAM_MAX_K];
  __shared__ int red_i[2][BEAM_THREADS / 64], sel_i[BEAM_MAX_K];

  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* base = scores + (long long)n * ld_n;

  for (int e = tid; e < K * C; e += BEAM_THREADS) folded[e] = 0;
  if (tid == 0) {
    s_pb[0][0] = 0.0;
    s_pnb[0][0] = -INFINITY;
    s_tot[0][0] = 0.0;
    s_hash[0][0] = BEAM_HASH_SEED;
    s_phash[0][0] = 0;
    s_len[0][0] = 0;
    s_last[0][0] = -1;
  }
  int g = 0, nlive = 1;
  float nxt = tid < C ? base[tid] : 0.f;

  for (int t = 0; t < T; ++t) {
    if (tid < C) row[tid] = nxt != nxt ? -INFINITY : (double)nxt;
    if (tid < K) parent[tid] = -1;
    __syncthreads();

    // slot 0 of every entry; which entries are another entry's prefix plus one token (hash first, the bytes decide)
    if (tid < nlive) {
      const int l = s_last[g][tid];
      stay_pb[tid] = s_tot[g][tid] + row[blank];
      stay_pnb[tid] = l >= 0 ? s_pnb[g][tid] + row[l] : -INFINITY;
    }
    for (int p = tid; p < nlive * nlive; p += BEAM_THREADS) {
      const int i = p / nlive, j = p - i * nlive;
      const int li = s_len[g][i];
      if (s_len[g][j] == li + 1 && s_phash[g][j] == s_hash[g][i]) {
        const unsigned char* a = pre + (size_t)(g * K + i) * T;
        const unsigned char* b = pre + (size_t)(g * K + j) * T;
        bool same = true;
        for (int q = 0; q < li; ++q) same = same && a[q] == b[q];
        if (same) parent[j] = i;                                        // prefixes are distinct: at most one i per j
      }
    }
    __syncthreads();

    // fold: entry i extended by last(j) IS entry j, so that mass joins j's stay slot and the slot of i disappears
    if (tid < nlive && parent[tid] >= 0) {
      const int i = parent[tid], c = s_last[g][tid];
      const double contrib = (c == s_last[g][i] ? s_pb[g][i] : s_tot[g][i]) + row[c];
      stay_pnb[tid] = beam_lse(stay_pnb[tid], contrib);
      folded[i * C + c] = 1;
    }
    __syncthreads();

    // candidate scores, in registers
    double sc[R];
    const int ncand = nlive * C;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int idx = r * BEAM_THREADS + tid;
      double v = -INFINITY;
      if (idx < ncand) {
        const int i = idx / C, s = idx - i * C;
        if (s == 0) {
          v = beam_lse(stay_pb[i], stay_pnb[i]);
        } else {
          const int c = beam_slot_class(s, blank);
          if (!folded[i * C + c]) v = (c == s_last[g][i] ? s_pb[g][i] : s_tot[g][i]) + row[c];
        }
        if (!(v > -INFINITY)) v = -INFINITY;                            // a NaN (from +inf inputs) is dropped like -inf
      }
      sc[r] = v;
    }
    if (t + 1 < T && tid < C) nxt = base[(long long)(t + 1) * ld_t + tid];   // next row: in flight during the selection

    double lb = -INFINITY;
    int lbi = INT_MAX;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (sc[r] > lb) {
        lb = sc[r];
        lbi = r * BEAM_THREADS + tid;
      }

    // K rounds of arg-max over (score, index); a round whose best is -inf ends the step with fewer than K entries
    int nnew = 0;
    for (int k = 0; k < K; ++k) {
      double bs = lb;
      int bi = lbi;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(bs, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (beam_before(os, oi, bs, bi)) {
          bs = os;
          bi = oi;
        }
      }
      if (lane == 0) {
        red_s[k & 1][wave] = bs;
        red_i[k & 1][wave] = bi;
      }
      __syncthreads();
      bs = red_s[k & 1][0];
      bi = red_i[k & 1][0];
#pragma unroll
      for (int w = 1; w < BEAM_THREADS / 64; ++w) {
        const double os = red_s[k & 1][w];
        const int oi = red_i[k & 1][w];
        if (beam_before(os, oi, bs, bi)) {
          bs = os;
          bi = oi;
        }
      }
      if (!(bs > -INFINITY)) break;                                     // the same value in every thread
      if (tid == 0) {
        sel_s[k] = bs;
        sel_i[k] = bi;
      }
      if ((bi & (BEAM_THREADS - 1)) == tid) {                           // the winner's owner takes it out and looks again
        const int wr = bi / BEAM_THREADS;
        lb = -INFINITY;
        lbi = INT_MAX;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (r == wr) sc[r] = -INFINITY;
          if (sc[r] > lb) {
            lb = sc[r];
            lbi = r * BEAM_THREADS + tid;
          }
        }
      }
      nnew = k + 1;
    }
    __syncthreads();

    if (tid < nlive && parent[tid] >= 0) folded[parent[tid] * C + s_last[g][tid]] = 0;   // the table is all zero between steps

    // the next generation
    const int g2 = g ^ 1;
    if (tid < nnew) {
      const int wi = sel_i[tid], i = wi / C, s = wi - i * C;
      if (s == 0) {
        s_pb[g2][tid] = stay_pb[i];
        s_pnb[g2][tid] = stay_pnb[i];
        s_hash[g2][tid] = s_hash[g][i];
        s_phash[g2][tid] = s_phash[g][i];
        s_len[g2][tid] = s_len[g][i];
        s_last[g2][tid] = s_last[g][i];
      } else {
        const int c = beam_slot_class(s, blank);
        s_pb[g2][tid] = -INFINITY;
        s_pnb[g2][tid] = sel_s[tid];
        s_hash[g2][tid] = (s_hash[g][i] ^ (unsigned long long)(c + 1)) * BEAM_HASH_MUL;
        s_phash[g2][tid] = s_hash[g][i];
        s_len[g2][tid] = s_len[g][i] + 1;
        s_last[g2][tid] = c;
      }
      s_tot[g2][tid] = sel_s[tid];                                      // lse(pb', pnb'): the candidate's score
    }
    const int L = t + 1;                                                // no prefix is longer than t + 1 after step t
    for (int e = tid; e < nnew * L; e += BEAM_THREADS) {
      const int k = e / L, q = e - k * L;
      const int wi = sel_i[k], i = wi / C, s = wi - i * C;
      const int ol = s_len[g][i];
      if (q < ol)
        pre[(size_t)(g2 * K + k) * T + q] = pre[(size_t)(g * K + i) * T + q];
      else if (q == ol && s != 0)
        pre[(size_t)(g2 * K + k) * T + q] = (unsigned char)beam_slot_class(s, blank);
    }
    __syncthreads();
    g = g2;
    nlive = nnew;
  }

  // the beam, in beam order; -1 behind every prefix and in the rows beyond the live count
  int* tok = tokens + (long long)n * K * T;
  for (int e = tid; e < K * T; e += BEAM_THREADS) {
    const int k = e / T, q = e - k * T;
    tok[e] = (k < nlive && q < s_len[g][k]) ? (int)pre[(size_t)(g * K + k) * T + q] : -1;
  }
  if (tid < K) {
    lengths[(long long)n * K + tid] = tid < nlive ? s_len[g][tid] : -1;
    beam_scores[(long long)n * K + tid] = tid < nlive ? s_tot[g][tid] : -INFINITY;
  }
}

template <int R>
void beam_launch(const float* scores, int ld_t, int ld_n, int T, int N, int C, int blank, int K, int* tokens, int* lengths, double* beam_scores,
                 hipStream_t stream) {
  hipLaunchKernelGGL(ctc_beam_kernel<R>, dim3(N), dim3(BEAM_THREADS), (size_t)2 * K * T, stream, scores, ld_t, ld_n, T, C, blank, K, tokens,
                     lengths, beam_scores);
}

}  // namespace

extern "C" int qea_ctc_beam_decode(const float* scores, int32_t ld_t, int32_t ld_n, int32_t T, int32_t N, int32_t C, int32_t blank, int32_t K,
                                   int32_t* tokens, int32_t* lengths, double* beam_scores, void* stream) {
  QEA_REQUIRE(scores && tokens && lengths && beam_scores && N > 0 && ld_t >= 0 && ld_n >= 0, "qea_ctc_beam_decode: bad arguments");
  QEA_REQUIRE(K >= 1 && K <= BEAM_MAX_K, "qea_ctc_beam_decode: K=%d outside 1..%d", K, BEAM_MAX_K);
  QEA_REQUIRE(C >= 2 && C <= BEAM_MAX_C, "qea_ctc_beam_decode: C=%d outside 2..%d", C, BEAM_MAX_C);
  QEA_REQUIRE(T >= 1 && T <= BEAM_MAX_T, "qea_ctc_beam_decode: T=%d outside 1..%d", T, BEAM_MAX_T);
  QEA_REQUIRE(blank >= 0 && blank < C, "qea_ctc_beam_decode: blank=%d outside 0..%d", blank, C - 1);
  const int per_thread = qea_cdiv((long long)K * C, BEAM_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (per_thread <= 1)
    beam_launch<1>(scores, ld_t, ld_n, T, N, C, blank, K, tokens, lengths, beam_scores, st);
  else if (per_thread <= 4)
    beam_launch<4>(scores, ld_t, ld_n, T, N, C, blank, K, tokens, lengths, beam_scores, st);
  else if (per_thread <= 12)
    beam_launch<12>(scores, ld_t, ld_n, T, N, C, blank, K, tokens, lengths, beam_scores, st);
  else
    beam_launch<32>(scores, ld_t, ld_n, T, N, C, blank, K, tokens, lengths, beam_scores, st);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
