// CTC forced alignment: the max-product (Viterbi) member of the family in ctc_core.h.  Given a label, the best single alignment of it to
// a sample's log-probs: its score, the character index of every step, the span of steps of every character and the sum of that
// character's log-probs over its span (DESIGN.md "Forced alignment"; include/qea_hip.h: qea_ctc_align).
//   v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), [v_{t-1}(s-2)]) + lp[t, l'_s]      first of equal candidates wins, its kind is the back-pointer
// fp64 adds and comparisons only: no exp, no log, so the device, qea/align.py and tests/align_spec.py agree bit for bit.
// One workgroup per sample, one thread per extended state (ctc_state of ctc_core.h), two prev rows in LDS and one barrier per step: the
// shape of ctc_scan.  (A second form for S <= 63, one wave per sample with the neighbour states moved by DPP wave shifts and no barrier
// in the time loop, was built and measured: 16.1 us against 17.5 us of device time at (T, N) = (31, 2048), and no difference at all
// through qea.ops, where the host needs 22.6 us to issue a call.  It was deleted: DESIGN.md, profiles/align.json.)
// Back-pointers are 2 bits; the owner thread packs 16 steps into a dword and stores it at bp[t / 16][thread]: consecutive lanes,
// consecutive banks.  After the loop thread 0 walks back through them into LDS (path as int8, first / last per character), then the
// workgroup stores the path coalesced and one thread per character adds its log-probs in ascending t.  Latency-bound: T dependent
// steps of one gather (fetched a step ahead), a max and an add.  Bytes: T * S * 4 gathered (whole rows are touched: T * C * 4 per
// sample), T * 4 + L * 16 + 8 stored.
#include "ctc_core.h"

namespace {

constexpr int ALIGN_MAX_T = 512, ALIGN_MAX_C = 256;

// a log-prob as the statement reads it: fp64 exactly, NaN and +inf as -inf
__device__ __forceinline__ double align_lp(float x) { return x < INFINITY ? (double)x : NEG_INF_D; }

// blockDim.x == ctc_scan_threads(2 L_max + 1), sample = blockIdx.x.  Dynamic LDS: ceil(T / 16) * blockDim.x dwords of back-pointers.
// No thread leaves before the last barrier.
__global__ __launch_bounds__(CTC_MAX_S) void ctc_align_kernel(const float* __restrict__ lp, int ld_t, int ld_n, const int* __restrict__ targets,
                                                              const long long* __restrict__ tg_off, int T, int C, int blank, int L_max,
                                                              double* __restrict__ score, int* __restrict__ path, int* __restrict__ first,
                                                              int* __restrict__ last, double* __restrict__ char_score) {
  extern __shared__ unsigned bp[];                 // [ceil(T / 16)][blockDim.x]
  __shared__ double prev[2][CTC_MAX_S + 2];        // cell s + 2 holds v(s); cells 0, 1 are the -inf the recursion reaches into
  __shared__ signed char pth[ALIGN_MAX_T];         // the path: -1..126
  __shared__ short sfirst[CTC_MAX_L + 1], slast[CTC_MAX_L + 1];
  const int nthr = blockDim.x;
  const int s = threadIdx.x;
  const int n = blockIdx.x;

  const long long off = tg_off[n];
  const long long len = tg_off[n + 1] - off;
  const bool fits = len >= 0 && len <= L_max;      // a label of 0..L_max characters
  const int L = fits ? (int)len : 0;
  const int* tg = targets + off;
  const int S = 2 * L + 1;
  int ch;
  bool skip;
  ctc_state(tg, s, S, blank, false, ch, skip);
  // a class that is no class, or the blank, inside the label: the sample is infeasible and the value never becomes an address
  const bool bad = (s < S) && (s & 1) && (ch < 0 || ch >= C || ch == blank);
  if (bad) ch = blank;
  const bool active = s < S;
  const float* lpn = lp + (size_t)n * ld_n + ch;

  double v = NEG_INF_D;
  if (active && s < 2) v = align_lp(lpn[0]);
  float nxt = (active && T > 1) ? lpn[(size_t)ld_t] : -INFINITY;
  unsigned word = 0;
  if (s < 2) prev[0][s] = prev[1][s] = NEG_INF_D;
  int buf = 0;
  prev[0][s + 2] = v;
  __syncthreads();
  for (int t = 1; t < T; ++t) {
    const float cur = nxt;
    if (active && t + 1 < T) nxt = lpn[(size_t)(t + 1) * ld_t];      // in flight across the barrier and the dependent max / add
    const double a1 = prev[buf][s + 1];
    const double a2 = skip ? prev[buf][s] : NEG_INF_D;
    double best = v;
    unsigned kind = 0;
    if (a1 > best) best = a1, kind = 1;
    if (a2 > best) best = a2, kind = 2;
    v = active ? best + align_lp(cur) : NEG_INF_D;
    word |= kind << (2 * (t & 15));
    if ((t & 15) == 15 || t == T - 1) {
      bp[(t >> 4) * nthr + s] = word;
      word = 0;
    }
    buf ^= 1;
    prev[buf][s + 2] = v;
    __syncthreads();
  }
  const bool any_bad = __syncthreads_or(bad) != 0;

  // the end (S - 1 wins a tie with S - 2), and the walk back by thread 0
  const double end1 = prev[buf][(S - 1) + 2];
  const double end2 = L >= 1 ? prev[buf][(S - 2) + 2] : NEG_INF_D;
  const double best = (fits && !any_bad) ? (end2 > end1 ? end2 : end1) : NEG_INF_D;
  const bool feasible = best > NEG_INF_D;
  if (s == 0) {
    score[n] = best;
    if (feasible) {
      int st = end2 > end1 ? S - 2 : S - 1;
      int above = -1;                              // the state of step t + 1
      for (int t = T - 1; t >= 0; --t) {
        const int k = (st & 1) ? (st >> 1) : -1;
        const int kind = t > 0 ? (int)((bp[(t >> 4) * nthr + st] >> (2 * (t & 15))) & 3u) : 0;
        pth[t] = (signed char)k;
        if (k >= 0) {
          if (above != st) slast[k] = (short)t;
          if (t == 0 || kind != 0) sfirst[k] = (short)t;
        }
        above = st;
        st -= kind;
      }
    }
  }
  __syncthreads();
  int* pn = path + (size_t)n * T;
  for (int t = s; t < T; t += nthr) pn[t] = feasible ? (int)pth[t] : -2;
  // the characters (all of them, also of a label longer than L_max: the arrays are target_offsets[N] long)
  for (long long k = s; k < len; k += nthr) {
    int f = -1, l = -1;
    double acc = NEG_INF_D;
    if (feasible) {
      f = sfirst[k];
      l = slast[k];
      const float* lpc = lp + (size_t)n * ld_n + tg[k];
      acc = align_lp(lpc[(size_t)f * ld_t]);
      for (int t = f + 1; t <= l; ++t) acc += align_lp(lpc[(size_t)t * ld_t]);
    }
    first[off + k] = f;
    last[off + k] = l;
    char_score[off + k] = acc;
  }
}

}  // namespace

extern "C" int qea_ctc_align(const float* scores, int32_t ld_t, int32_t ld_n, const int32_t* targets, const int64_t* target_offsets, int32_t T,
                             int32_t N, int32_t C, int32_t blank, int32_t L_max, double* score, int32_t* path, int32_t* first, int32_t* last,
                             double* char_score, void* stream) {
  QEA_REQUIRE(N >= 0 && ld_t >= 0 && ld_n >= 0, "qea_ctc_align: N=%d, ld_t=%d, ld_n=%d must not be negative", N, ld_t, ld_n);
  QEA_REQUIRE(T >= 1 && T <= ALIGN_MAX_T, "qea_ctc_align: T=%d outside 1..%d", T, ALIGN_MAX_T);
  QEA_REQUIRE(C >= 2 && C <= ALIGN_MAX_C, "qea_ctc_align: C=%d outside 2..%d", C, ALIGN_MAX_C);
  QEA_REQUIRE(blank >= 0 && blank < C, "qea_ctc_align: blank=%d outside 0..%d", blank, C - 1);
  if (const int rc = ctc_check_l_max("qea_ctc_align", L_max)) return rc;
  if (N == 0) return QEA_OK;
  QEA_REQUIRE(scores && targets && target_offsets && score && path && first && last && char_score, "qea_ctc_align: null pointer");
  const int threads = ctc_scan_threads(2 * L_max + 1);
  const size_t lds = (size_t)((T + 15) / 16) * threads * sizeof(unsigned);
  hipLaunchKernelGGL(ctc_align_kernel, dim3((unsigned)N), dim3(threads), lds, (hipStream_t)stream, scores, ld_t, ld_n, targets,
                     (const long long*)target_offsets, T, C, blank, L_max, score, path, first, last, char_score);
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}
