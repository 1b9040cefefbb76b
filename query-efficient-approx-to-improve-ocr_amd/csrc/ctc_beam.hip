// CTC prefix beam search (include/qea_hip.h: qea_ctc_beam_decode, qea_ctc_beam_decode_lm, qea_ctc_beam_decode_dfa; the specification is
// DESIGN.md "CTC prefix beam search", "Character n-gram fusion" and "Automaton-constrained search").
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
//
// LM = true (qea_ctc_beam_decode_lm) is the same body with a character n-gram prior fused in: an entry also carries lm (the sum of the
// fused-table entries along its prefix) and ctx (the index of its last m tokens), the candidate registers hold the RANKING score
// (CTC term + lm, table entries are only ever added), and the next generation's pb / pnb / tot are recomputed from the CTC terms,
// never derived from the ranking score.  LM = false compiles to the plain search: every fused statement is under if constexpr.
//
// DFA = true (qea_ctc_beam_decode_dfa, MODE = BEAM_DFA) is the plain search restricted to the paths of a deterministic automaton in CSR
// form (first / label / child): an entry also carries its state and that state's edge range [lo, hi), clamped to 0..E.  Per step the
// threads walk the edge lists of the live entries laid end to end, 256 edges at a time (the live states of a trie seldom have more
// between them: one round trip of label and child) and mark the slots that exist with a 2 in the `folded` table; a fold overwrites
// the mark with 1, the slot's one reader clears the byte, so the table is still all zero between steps.  For the first edge it
// walked a thread also reads first[child], first[child + 1] and keeps the candidate index, the child and that range: the loads have
// long arrived when the selection ends, and the thread whose candidate won writes the new entry's state without another load (edges
// behind the first 256 are walked a second time for this).  Nothing here depends on R, and the scores stay pure CTC quantities.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int BEAM_THREADS = 256;
constexpr int BEAM_MAX_K = 32, BEAM_MAX_C = 256, BEAM_MAX_T = 512;
constexpr int BEAM_PLAIN = 0, BEAM_LM = 1, BEAM_DFA = 2;              // the compile-time modes of ctc_beam_kernel
constexpr int BEAM_LM_MAX_CONTEXT = 2;
constexpr int BEAM_DFA_MAX_E = (1 << 26) - 1;                           // K edge lists end to end are counted in an int: 32 * E < 2^31
constexpr long long BEAM_LM_MAX_ENTRIES = 1ll << 21;                    // C^(m+1) fp64 entries: 16 MB
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

// a fused-table entry: NaN counts as -inf
__device__ __forceinline__ double beam_lm_entry(const double* __restrict__ lm_table, int ctx, int C, int c) {
  const double w = lm_table[(long long)ctx * C + c];
  return w != w ? -INFINITY : w;
}

// an index of `first` as an edge offset: clamped to 0..E
__device__ __forceinline__ int beam_edge_bound(const int* __restrict__ first, int st, int E) { return min(max(first[st], 0), E); }

// Edge number q of the live entries' edge lists [lo_i, hi_i) laid end to end, q below their total: its entry i and its index e.
__device__ __forceinline__ int beam_dfa_entry(int q, int nlive, const int* lo, const int* hi, int& e) {
  int before = 0, i = 0;
  for (; i < nlive - 1; ++i) {
    const int deg = max(hi[i] - lo[i], 0);
    if (q < before + deg) break;
    before += deg;
  }
  e = lo[i] + (q - before);
  return i;
}

// The class and the child of edge e; the class is -1 for an edge that is absent (a label that is the blank or outside 0..C-1, a child
// outside 0..S-1).
__device__ __forceinline__ int beam_dfa_class(const int* __restrict__ label, const int* __restrict__ child, int e, int C, int blank, int S,
                                              int& ch) {
  const int c = label[e];
  ch = child[e];
  return (c >= 0 && c < C && c != blank && ch >= 0 && ch < S) ? c : -1;
}

// R: candidate registers per thread, K * C <= R * 256.  LM: lm_table [ctx_mod][C] fp64 with ctx_mod = C^m, total_scores [N][K];
// without LM the three are unused (NULL, 1, NULL).  DFA: first [S + 1], label [E], child [E], states [N][K]; without DFA unused
// (NULL, NULL, NULL, 0, 0, NULL).
// A workgroup is one wave per SIMD, so waves per SIMD = workgroups per CU, and with 8 strips per CU (N = 2048) a variant that loses
// one takes another round.  The plain variants fit 5, 4, 2, 1 (94, 124, 205, 256 + AGPRs); left alone the fused ones take 104, 141,
// 245 + 32 AGPRs (the table entries' addresses) and fit 4, 3, 1, 1: they are asked to keep the plain variants' occupancy.
// The automaton variants, left alone, take 110, 137, 217 and fit 4, 3, 2, 1; R = 4 (the workload's K = 8, C = 95) is asked for the plain
// variant's 4 and gets there (127) without scratch, R = 1 (K * C <= 256) spills 32 bytes at 5 and is asked for 4.
constexpr int beam_min_waves(int R, int MODE) { return MODE == BEAM_PLAIN ? 1 : R == 1 ? (MODE == BEAM_LM ? 5 : 4) : R == 4 ? 4 : R == 12 ? 2 : 1; }

template <int R, int MODE>
__global__ __launch_bounds__(BEAM_THREADS, beam_min_waves(R, MODE)) void ctc_beam_kernel(
    const float* __restrict__ scores, int ld_t, int ld_n, int T, int C, int blank, int K, const double* __restrict__ lm_table, int ctx_mod,
    int* __restrict__ tokens, int* __restrict__ lengths, double* __restrict__ beam_scores, double* __restrict__ total_scores,
    const int* __restrict__ first, const int* __restrict__ label, const int* __restrict__ child, int S, int E, int* __restrict__ states) {
  constexpr bool LM = MODE == BEAM_LM, DFA = MODE == BEAM_DFA;
  extern __shared__ __align__(16) unsigned char pre[];                 // [2][K][T] prefixes, one byte per token
  __shared__ double row[BEAM_MAX_C];                                    // lp[t][:] as fp64, NaN -> -inf
  __shared__ double s_pb[2][BEAM_MAX_K], s_pnb[2][BEAM_MAX_K], s_tot[2][BEAM_MAX_K];
  __shared__ unsigned long long s_hash[2][BEAM_MAX_K], s_phash[2][BEAM_MAX_K];
  __shared__ int s_len[2][BEAM_MAX_K], s_last[2][BEAM_MAX_K];
  __shared__ double s_lm[2][BEAM_MAX_K];                                // LM: the table entries along the prefix, added up
  __shared__ int s_ctx[2][BEAM_MAX_K];                                  // LM: index of the last m tokens, BOS (= blank) padded
  __shared__ int s_state[2][BEAM_MAX_K], s_lo[2][BEAM_MAX_K], s_hi[2][BEAM_MAX_K];   // DFA: the state, its edges [lo, hi) within 0..E
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
    if constexpr (LM) {
      int ctx = 0;
      for (int q = 1; q < ctx_mod; q *= C) ctx = ctx * C + blank;       // the blank, m times
      s_lm[0][0] = 0.0;
      s_ctx[0][0] = ctx;
    }
    if constexpr (DFA) {
      s_state[0][0] = 0;
      s_lo[0][0] = beam_edge_bound(first, 0, E);
      s_hi[0][0] = beam_edge_bound(first, 1, E);
    }
  }
  int g = 0, nlive = 1;
  float nxt = tid < C ? base[tid] : 0.f;

  for (int t = 0; t < T; ++t) {
    if (tid < C) row[tid] = nxt != nxt ? -INFINITY : (double)nxt;
    if (tid < K) parent[tid] = -1;
    __syncthreads();

    // LM: the table entry of every extension slot this thread owns; in flight during the stay slots and the folding
    // (they wait in the candidate registers: consecutive threads read consecutive classes of one table row)
    double sc[R];
    if constexpr (LM) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int idx = r * BEAM_THREADS + tid;
        sc[r] = 0.0;
        if (idx < nlive * C) {
          const int i = idx / C, s = idx - i * C;
          if (s != 0) sc[r] = beam_lm_entry(lm_table, s_ctx[g][i], C, beam_slot_class(s, blank));
        }
      }
    }

    // DFA: the slots that exist.  The edge lists of the live entries, end to end, are walked 256 edges at a time (a trie's live states
    // seldom have more between them: one round trip).  For edge number tid a thread keeps the candidate index, the child and the
    // child's own edge range, read here so that it has arrived long before the selection ends: a winner then needs no load at all.
    int my_cand = -1, my_state = 0, my_lo = 0, my_hi = 0, nedges = 0;
    if constexpr (DFA) {
      int i0 = 0, before = 0;
      for (int i = 0; i < nlive; ++i) {                                 // one pass: the number of edges and the entry of edge number tid
        nedges += max(s_hi[g][i] - s_lo[g][i], 0);
        if (tid >= nedges) {
          i0 = i + 1;
          before = nedges;
        }
      }
      if (tid < nedges) {
        int ch;
        const int c = beam_dfa_class(label, child, s_lo[g][i0] + (tid - before), C, blank, S, ch);
        if (c >= 0) {
          folded[i0 * C + c] = 2;
          my_cand = i0 * C + (c < blank ? c + 1 : c);
          my_state = ch;
          my_lo = first[ch];
          my_hi = first[ch + 1];
        }
      }
      for (int q = tid + BEAM_THREADS; q < nedges; q += BEAM_THREADS) {
        int e, ch;
        const int i = beam_dfa_entry(q, nlive, s_lo[g], s_hi[g], e), c = beam_dfa_class(label, child, e, C, blank, S, ch);
        if (c >= 0) folded[i * C + c] = 2;
      }
    }

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
    const int ncand = nlive * C;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int idx = r * BEAM_THREADS + tid;
      double v = -INFINITY;
      if (idx < ncand) {
        const int i = idx / C, s = idx - i * C;
        if (s == 0) {
          v = beam_lse(stay_pb[i], stay_pnb[i]);
          if constexpr (LM) v = v + s_lm[g][i];
        } else {
          const int c = beam_slot_class(s, blank);
          bool exists;
          if constexpr (DFA) {                                          // marked and not folded; this slot's one reader clears the byte
            const unsigned char f = folded[i * C + c];
            if (f) folded[i * C + c] = 0;
            exists = f == 2;
          } else {
            exists = !folded[i * C + c];
          }
          if (exists) {
            v = (c == s_last[g][i] ? s_pb[g][i] : s_tot[g][i]) + row[c];
            if constexpr (LM) {
              const double lm2 = s_lm[g][i] + sc[r];                    // first lm', then the sum: the specification's association
              v = v + lm2;
            }
          }
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

    if constexpr (!DFA)
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
        if constexpr (LM) {
          s_tot[g2][tid] = beam_lse(stay_pb[i], stay_pnb[i]);
          s_lm[g2][tid] = s_lm[g][i];
          s_ctx[g2][tid] = s_ctx[g][i];
        }
      } else {
        const int c = beam_slot_class(s, blank);
        s_pb[g2][tid] = -INFINITY;
        if constexpr (LM) {                                             // sel_s is the ranking score: the CTC term is formed again
          const double pnb = (c == s_last[g][i] ? s_pb[g][i] : s_tot[g][i]) + row[c];
          s_pnb[g2][tid] = pnb;
          s_tot[g2][tid] = pnb;
          s_lm[g2][tid] = s_lm[g][i] + beam_lm_entry(lm_table, s_ctx[g][i], C, c);
          s_ctx[g2][tid] = (s_ctx[g][i] * C + c) % ctx_mod;
        } else {
          s_pnb[g2][tid] = sel_s[tid];
        }
        s_hash[g2][tid] = (s_hash[g][i] ^ (unsigned long long)(c + 1)) * BEAM_HASH_MUL;
        s_phash[g2][tid] = s_hash[g][i];
        s_len[g2][tid] = s_len[g][i] + 1;
        s_last[g2][tid] = c;
      }
      if constexpr (!LM) s_tot[g2][tid] = sel_s[tid];                   // lse(pb', pnb'): the candidate's score
    }
    // DFA: a stay keeps its state; the edge of an extension is found by the walk that marked it, its finder reads the child's range
    if constexpr (DFA) {
      if (tid < nnew) {
        const int wi = sel_i[tid], i = wi / C;
        if (wi - i * C == 0) {
          s_state[g2][tid] = s_state[g][i];
          s_lo[g2][tid] = s_lo[g][i];
          s_hi[g2][tid] = s_hi[g][i];
        }
      }
      if (my_cand >= 0)
        for (int k = 0; k < nnew; ++k)
          if (sel_i[k] == my_cand) {                                    // this thread's candidate won: its edge names the state
            s_state[g2][k] = my_state;
            s_lo[g2][k] = min(max(my_lo, 0), E);
            s_hi[g2][k] = min(max(my_hi, 0), E);
          }
      for (int q = tid + BEAM_THREADS; q < nedges; q += BEAM_THREADS) {   // the edges behind the first 256: walked again
        int e, ch;
        const int i = beam_dfa_entry(q, nlive, s_lo[g], s_hi[g], e), c = beam_dfa_class(label, child, e, C, blank, S, ch);
        if (c < 0) continue;
        const int cand = i * C + (c < blank ? c + 1 : c);
        for (int k = 0; k < nnew; ++k)
          if (sel_i[k] == cand) {
            s_state[g2][k] = ch;
            s_lo[g2][k] = beam_edge_bound(first, ch, E);
            s_hi[g2][k] = beam_edge_bound(first, ch + 1, E);
          }
      }
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
    if constexpr (LM) total_scores[(long long)n * K + tid] = tid < nlive ? s_tot[g][tid] + s_lm[g][tid] : -INFINITY;
    if constexpr (DFA) states[(long long)n * K + tid] = tid < nlive ? s_state[g][tid] : -1;
  }
}

// what only one of the modes reads: the fused table, the automaton
struct BeamExtra {
  const double* lm_table = nullptr;
  int ctx_mod = 1;
  double* total_scores = nullptr;
  const int *first = nullptr, *label = nullptr, *child = nullptr;
  int S = 0, E = 0;
  int* states = nullptr;
};

template <int R, int MODE>
void beam_launch(const float* scores, int ld_t, int ld_n, int T, int N, int C, int blank, int K, const BeamExtra& x, int* tokens,
                 int* lengths, double* beam_scores, hipStream_t stream) {
  hipLaunchKernelGGL((ctc_beam_kernel<R, MODE>), dim3(N), dim3(BEAM_THREADS), (size_t)2 * K * T, stream, scores, ld_t, ld_n, T, C, blank, K,
                     x.lm_table, x.ctx_mod, tokens, lengths, beam_scores, x.total_scores, x.first, x.label, x.child, x.S, x.E, x.states);
}

// the limits the entry points share, then the register variant that holds K * C candidates
template <int MODE>
int beam_decode(const char* who, const float* scores, int ld_t, int ld_n, int T, int N, int C, int blank, int K, const BeamExtra& x,
                int* tokens, int* lengths, double* beam_scores, hipStream_t st) {
  QEA_REQUIRE(scores && tokens && lengths && beam_scores && N > 0 && ld_t >= 0 && ld_n >= 0, "%s: bad arguments", who);
  QEA_REQUIRE(K >= 1 && K <= BEAM_MAX_K, "%s: K=%d outside 1..%d", who, K, BEAM_MAX_K);
  QEA_REQUIRE(C >= 2 && C <= BEAM_MAX_C, "%s: C=%d outside 2..%d", who, C, BEAM_MAX_C);
  QEA_REQUIRE(T >= 1 && T <= BEAM_MAX_T, "%s: T=%d outside 1..%d", who, T, BEAM_MAX_T);
  QEA_REQUIRE(blank >= 0 && blank < C, "%s: blank=%d outside 0..%d", who, blank, C - 1);
  const int per_thread = qea_cdiv((long long)K * C, BEAM_THREADS);
  if (per_thread <= 1)
    beam_launch<1, MODE>(scores, ld_t, ld_n, T, N, C, blank, K, x, tokens, lengths, beam_scores, st);
  else if (per_thread <= 4)
    beam_launch<4, MODE>(scores, ld_t, ld_n, T, N, C, blank, K, x, tokens, lengths, beam_scores, st);
  else if (per_thread <= 12)
    beam_launch<12, MODE>(scores, ld_t, ld_n, T, N, C, blank, K, x, tokens, lengths, beam_scores, st);
  else
    beam_launch<32, MODE>(scores, ld_t, ld_n, T, N, C, blank, K, x, tokens, lengths, beam_scores, st);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

}  // namespace

extern "C" int qea_ctc_beam_decode(const float* scores, int32_t ld_t, int32_t ld_n, int32_t T, int32_t N, int32_t C, int32_t blank, int32_t K,
                                   int32_t* tokens, int32_t* lengths, double* beam_scores, void* stream) {
  return beam_decode<BEAM_PLAIN>("qea_ctc_beam_decode", scores, ld_t, ld_n, T, N, C, blank, K, BeamExtra{}, tokens, lengths, beam_scores,
                                 (hipStream_t)stream);
}

extern "C" int qea_ctc_beam_decode_lm(const float* scores, int32_t ld_t, int32_t ld_n, int32_t T, int32_t N, int32_t C, int32_t blank, int32_t K,
                                      const double* lm_table, int32_t lm_context, int32_t* tokens, int32_t* lengths, double* ctc_scores,
                                      double* total_scores, void* stream) {
  QEA_REQUIRE(lm_table && total_scores, "qea_ctc_beam_decode_lm: bad arguments");
  QEA_REQUIRE(lm_context >= 0 && lm_context <= BEAM_LM_MAX_CONTEXT, "qea_ctc_beam_decode_lm: lm_context=%d outside 0..%d", lm_context,
              BEAM_LM_MAX_CONTEXT);
  QEA_REQUIRE(C >= 2 && C <= BEAM_MAX_C, "qea_ctc_beam_decode_lm: C=%d outside 2..%d", C, BEAM_MAX_C);
  long long ctx_mod = 1;
  for (int q = 0; q < lm_context; ++q) ctx_mod *= C;
  QEA_REQUIRE(ctx_mod * C <= BEAM_LM_MAX_ENTRIES, "qea_ctc_beam_decode_lm: a table of C^(m+1) = %lld entries, more than %lld", ctx_mod * C,
              BEAM_LM_MAX_ENTRIES);
  BeamExtra x;
  x.lm_table = lm_table;
  x.ctx_mod = (int)ctx_mod;
  x.total_scores = total_scores;
  return beam_decode<BEAM_LM>("qea_ctc_beam_decode_lm", scores, ld_t, ld_n, T, N, C, blank, K, x, tokens, lengths, ctc_scores, (hipStream_t)stream);
}

extern "C" int qea_ctc_beam_decode_dfa(const float* scores, int32_t ld_t, int32_t ld_n, int32_t T, int32_t N, int32_t C, int32_t blank, int32_t K,
                                       const int32_t* first, const int32_t* label, const int32_t* child, int32_t S, int32_t E, int32_t* tokens,
                                       int32_t* lengths, double* beam_scores, int32_t* states, void* stream) {
  QEA_REQUIRE(first && label && child && states, "qea_ctc_beam_decode_dfa: bad arguments");
  QEA_REQUIRE(S >= 1 && E >= 0 && E <= BEAM_DFA_MAX_E, "qea_ctc_beam_decode_dfa: S=%d states (at least 1), E=%d edges (0..%d)", S, E,
              BEAM_DFA_MAX_E);
  BeamExtra x;
  x.first = first;
  x.label = label;
  x.child = child;
  x.S = S;
  x.E = E;
  x.states = states;
  return beam_decode<BEAM_DFA>("qea_ctc_beam_decode_dfa", scores, ld_t, ld_n, T, N, C, blank, K, x, tokens, lengths, beam_scores,
                               (hipStream_t)stream);
}
