// Greedy facility-location selection (pruning/methods.py `facility_location`): k picks over n feature rows of d doubles.
//
//   S[i][j] = M - sum_dd (x[i][dd] - x[j][dd])^2        M = the largest squared distance over all pairs
//   cur[j]  = 0;   pick t: w = argmax over unpicked i of gain[i] = sum_j max(S[i][j], cur[j])   (lowest index on an exact tie)
//                          cur[j] = max(cur[j], S[w][j])
//
// S is never stored: every pick recomputes the n x n pair terms from x (fp64 vector ALU; at d = 1 five operations per pair for the
// term and three for its error-free accumulation).
// Two launches per pick, enqueued back to back with no host synchronisation: fl_pairs_kernel<FL_GAIN> (one wave = FL_CAND candidates
// against all j) and fl_select_kernel (one workgroup: arg-max, output, cur update).  No workgroup waits for another one.
//
// Every term is rounded exactly as written here (no fused multiply-add: `fp contract(off)`), so a host replay that evaluates the same
// expressions in fp64 gets the same TERMS bit for bit and differs only in how it sums them over j.  Here that order is fixed and is a
// function of j alone: lane l of a wave adds j = l, l + 64, l + 128, ... in ascending order, then the 64 lane sums meet in an xor
// butterfly (32, 16, ..., 1; symmetric in its two inputs, so all lanes hold one value).  Rows with identical features therefore get
// bit-identical gains and the index decides.
//
// The sum is COMPENSATED (a high word and the exact rounding errors of its additions in a low word, added once at the end), because
// CER tables sit on a lattice (multiples of 0.001): candidates with DIFFERENT features routinely have gains whose exact sums are
// equal (picks 27, 77, 90, 103 and 130 of the POS ranking), and a plain fp64 sum decides such a tie by its own rounding, one way on
// one summation order and the other way on the next.  With the error words carried, equal exact sums give equal gains and the tie
// rule (lowest index) decides, as it does in the recorded reference ranking.
#include "common.h"
#include <float.h>
#include <limits.h>

namespace {

constexpr int FL_CAND = 4;              // candidates per wave, accumulators in registers
constexpr int FL_WAVES = 4;             // waves per workgroup: 16 candidates share one staged tile of x_j / cur_j
constexpr int FL_THREADS = FL_WAVES * QEA_WAVE;
constexpr int FL_BLOCK_CAND = FL_CAND * FL_WAVES;
constexpr int FL_JT_D1 = 1024;          // j per LDS tile, d = 1 (16 KB; next tile prefetched into registers)
constexpr int FL_JT_DN = 128;           // j per LDS tile, 2 <= d <= 32 ((128 * 33 + 16 * 32) * 8 = 37 KB at d = 32)
constexpr int FL_MAX_D = 32;
constexpr int FL_SELECT_THREADS = 1024;

enum { FL_MAXDIST = 0, FL_GAIN = 1 };
enum { FL_FLAG_NONFINITE = 1, FL_FLAG_OVERFLOW = 2, FL_FLAG_NO_WINNER = 4 };

// workspace: [int32 flag][int32 pad][u64 bits of M][cur: n doubles][gain: n doubles][picked: n int32]
struct FlWorkspace {
  int* flag;
  unsigned long long* m_bits;
  double* cur;
  double* gain;
  int* picked;
};

FlWorkspace fl_carve(void* ws, int n) {
  char* p = (char*)ws;
  FlWorkspace w;
  w.flag = (int*)p;
  w.m_bits = (unsigned long long*)(p + 8);
  w.cur = (double*)(p + 16);
  w.gain = w.cur + n;
  w.picked = (int*)(w.gain + n);
  return w;
}

__device__ __forceinline__ double fl_wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// a + b = s + e exactly (Knuth), any magnitudes; symmetric in a and b
__device__ __forceinline__ void fl_two_sum(double a, double b, double& s, double& e) {
#pragma clang fp contract(off)
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

__device__ __forceinline__ bool fl_finite(double v) { return fabs(v) <= DBL_MAX; }   // false for NaN and +-inf

// One wave: FL_CAND candidates i against every j; MODE FL_MAXDIST folds the squared distances into M (one integer atomicMax per
// wave: non-negative doubles order like their bit patterns) and raises the non-finite flag, MODE FL_GAIN writes gain[i].
template <int MODE, bool D1>
__global__ __launch_bounds__(FL_THREADS) void fl_pairs_kernel(const double* __restrict__ x, int n, int d, const double* __restrict__ cur,
                                                              int* __restrict__ flag, unsigned long long* __restrict__ m_bits,
                                                              double* __restrict__ gain) {
#pragma clang fp contract(off)
  constexpr int JT = D1 ? FL_JT_D1 : FL_JT_DN;
  extern __shared__ double fl_smem[];
  double* xs = fl_smem;                         // [d][JT]
  double* cs = xs + (size_t)d * JT;             // [JT]
  double* xc = cs + JT;                         // [FL_BLOCK_CAND][d] (d > 1 only)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double M = 0.0;
  if (MODE == FL_GAIN) {
    if (*flag) return;                          // the whole grid takes this branch: nothing below runs on refused input
    M = __longlong_as_double((long long)*m_bits);
  }
  const int i0 = blockIdx.x * FL_BLOCK_CAND + wave * FL_CAND;
  double xi[FL_CAND], acc[FL_CAND], lo[FL_CAND];
  int bad = 0;
#pragma unroll
  for (int c = 0; c < FL_CAND; ++c) {
    // FL_GAIN: the high word starts at M >= every term (S <= M, cur <= M), so |acc| >= |term| holds for each addition and its
    // rounding error is (term - (sum - acc)) exactly (Dekker's fast two-sum); the offset comes off again after the loop
    acc[c] = M;
    lo[c] = 0.0;
    xi[c] = D1 ? x[min(i0 + c, n - 1)] : 0.0;   // rows past n repeat row n-1; their results are not written
  }
  if (!D1) {
    for (int e = tid; e < FL_BLOCK_CAND * d; e += FL_THREADS) {
      const int row = min(blockIdx.x * FL_BLOCK_CAND + e / d, n - 1);
      xc[e] = x[(size_t)row * d + e % d];
    }
  }
  constexpr int PRE = FL_JT_D1 / FL_THREADS;    // d = 1: elements of the next tile each thread holds in registers
  double px[PRE], pc[PRE];
  if (D1) {
#pragma unroll
    for (int r = 0; r < PRE; ++r) {
      const int j = tid + r * FL_THREADS;
      px[r] = j < n ? x[j] : 0.0;
      pc[r] = (MODE == FL_GAIN && j < n) ? cur[j] : 0.0;
    }
  }
  for (int j0 = 0; j0 < n; j0 += JT) {
    __syncthreads();                            // the previous tile has been read by every wave
    if (D1) {
#pragma unroll
      for (int r = 0; r < PRE; ++r) {
        xs[tid + r * FL_THREADS] = px[r];
        cs[tid + r * FL_THREADS] = pc[r];
        if (MODE == FL_MAXDIST && !fl_finite(px[r])) bad |= FL_FLAG_NONFINITE;
      }
#pragma unroll
      for (int r = 0; r < PRE; ++r) {
        const int j = j0 + JT + tid + r * FL_THREADS;
        px[r] = j < n ? x[j] : 0.0;
        pc[r] = (MODE == FL_GAIN && j < n) ? cur[j] : 0.0;
      }
    } else {
      for (int e = tid; e < JT * d; e += FL_THREADS) {
        const int jl = e / d, dd = e - jl * d;
        const double v = (j0 + jl < n) ? x[(size_t)(j0 + jl) * d + dd] : 0.0;
        xs[dd * JT + jl] = v;
        if (MODE == FL_MAXDIST && !fl_finite(v)) bad |= FL_FLAG_NONFINITE;
      }
      if (MODE == FL_GAIN)
        for (int jl = tid; jl < JT; jl += FL_THREADS) cs[jl] = (j0 + jl < n) ? cur[j0 + jl] : 0.0;
    }
    __syncthreads();
    const int jend = min(JT, n - j0);
#pragma unroll 4
    for (int jl = lane; jl < jend; jl += QEA_WAVE) {
      double dist[FL_CAND];
      if (D1) {
        const double xj = xs[jl];
#pragma unroll
        for (int c = 0; c < FL_CAND; ++c) {
          const double df = xi[c] - xj;
          dist[c] = df * df;
        }
      } else {
#pragma unroll
        for (int c = 0; c < FL_CAND; ++c) dist[c] = 0.0;
        for (int dd = 0; dd < d; ++dd) {
          const double xj = xs[dd * JT + jl];
#pragma unroll
          for (int c = 0; c < FL_CAND; ++c) {
            const double df = xc[(wave * FL_CAND + c) * d + dd] - xj;
            dist[c] = dist[c] + df * df;
          }
        }
      }
      if (MODE == FL_MAXDIST) {
#pragma unroll
        for (int c = 0; c < FL_CAND; ++c) acc[c] = fmax(acc[c], dist[c]);
      } else {
        const double cj = cs[jl];
#pragma unroll
        for (int c = 0; c < FL_CAND; ++c) {
          const double term = fmax(M - dist[c], cj);
          const double sum = acc[c] + term;
          lo[c] = lo[c] + (term - (sum - acc[c]));
          acc[c] = sum;
        }
      }
    }
  }
  if (MODE == FL_MAXDIST) {
    double m = fmax(fmax(acc[0], acc[1]), fmax(acc[2], acc[3]));
    m = fl_wave_max_d(m);
    if (!fl_finite(m)) bad |= FL_FLAG_OVERFLOW;            // finite features whose squared distance overflows
    if (bad) atomicOr(flag, bad);
    if (lane == 0 && fl_finite(m)) atomicMax(m_bits, (unsigned long long)__double_as_longlong(m));
  } else {
#pragma unroll
    for (int c = 0; c < FL_CAND; ++c) {
      double hi, e;
      fl_two_sum(acc[c], -M, hi, e);
      double low = lo[c] + e;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ohi = __shfl_xor(hi, o, 64), olow = __shfl_xor(low, o, 64);
        fl_two_sum(hi, ohi, hi, e);
        low = (low + olow) + e;
      }
      if (lane == 0 && i0 + c < n) gain[i0 + c] = hi + low;
    }
  }
}

// (value, index) ordering of the arg-max: larger value first, then the lower index
__device__ __forceinline__ void fl_better(double& v, int& i, double ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// One workgroup: pick t = the unpicked candidate with the largest gain, write it out, fold its similarities into cur.
__global__ __launch_bounds__(FL_SELECT_THREADS) void fl_select_kernel(const double* __restrict__ x, int n, int d, int t,
                                                                      double* __restrict__ cur, const double* __restrict__ gain,
                                                                      int* __restrict__ picked, int* __restrict__ flag,
                                                                      const unsigned long long* __restrict__ m_bits,
                                                                      int32_t* __restrict__ ranking_out, double* __restrict__ gain_out) {
#pragma clang fp contract(off)
  __shared__ double sv[FL_SELECT_THREADS / QEA_WAVE];
  __shared__ int si[FL_SELECT_THREADS / QEA_WAVE];
  if (*flag) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double bv = -1.0;                                        // gains are sums of non-negative terms
  int bi = INT_MAX;
  for (int i = tid; i < n; i += FL_SELECT_THREADS)
    if (!picked[i]) fl_better(bv, bi, gain[i], i);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    fl_better(bv, bi, ov, oi);
  }
  if (lane == 0) {
    sv[wave] = bv;
    si[wave] = bi;
  }
  __syncthreads();
  bv = sv[0];
  bi = si[0];
  for (int w = 1; w < FL_SELECT_THREADS / QEA_WAVE; ++w) fl_better(bv, bi, sv[w], si[w]);
  if (bi < 0 || bi >= n) {                                 // cannot happen with finite gains and t < n; never index with it
    if (tid == 0) atomicOr(flag, FL_FLAG_NO_WINNER);
    return;
  }
  if (tid == 0) {
    ranking_out[t] = bi;
    if (gain_out) gain_out[t] = bv;
    picked[bi] = 1;
  }
  const double M = __longlong_as_double((long long)*m_bits);
  const double* xw = x + (size_t)bi * d;
  for (int j = tid; j < n; j += FL_SELECT_THREADS) {
    double dist = 0.0;
    for (int dd = 0; dd < d; ++dd) {
      const double df = xw[dd] - x[(size_t)j * d + dd];
      dist = dist + df * df;
    }
    cur[j] = fmax(cur[j], M - dist);
  }
}

size_t fl_lds_bytes(int d) {
  return d == 1 ? (size_t)2 * FL_JT_D1 * sizeof(double) : ((size_t)(d + 1) * FL_JT_DN + (size_t)FL_BLOCK_CAND * d) * sizeof(double);
}

template <int MODE>
void fl_launch_pairs(const double* x, int n, int d, const FlWorkspace& w, hipStream_t s) {
  const dim3 grid(qea_cdiv(n, FL_BLOCK_CAND)), block(FL_THREADS);
  if (d == 1)
    hipLaunchKernelGGL((fl_pairs_kernel<MODE, true>), grid, block, fl_lds_bytes(d), s, x, n, d, w.cur, w.flag, w.m_bits, w.gain);
  else
    hipLaunchKernelGGL((fl_pairs_kernel<MODE, false>), grid, block, fl_lds_bytes(d), s, x, n, d, w.cur, w.flag, w.m_bits, w.gain);
}

}  // namespace

extern "C" size_t qea_facility_workspace_bytes(int32_t n, int32_t d) {
  if (n < 1 || d < 1 || d > FL_MAX_D) return 0;
  return (16 + (size_t)n * 20 + 15) & ~(size_t)15;
}

extern "C" int qea_facility_select(const double* x, int32_t n, int32_t d, int32_t k, int32_t* ranking_out, double* gain_out, void* workspace,
                                   void* stream) {
  QEA_REQUIRE(x && ranking_out && workspace, "qea_facility_select: null pointer (x, ranking_out and workspace are required)");
  QEA_REQUIRE(d >= 1 && d <= FL_MAX_D, "qea_facility_select: d=%d outside 1..%d", d, FL_MAX_D);
  QEA_REQUIRE(n >= 1 && (long long)n * d < (1ll << 31), "qea_facility_select: n=%d rows of d=%d not supported", n, d);
  QEA_REQUIRE(k >= 1 && k <= n, "qea_facility_select: k=%d outside 1..n=%d", k, n);
  QEA_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)x & 7) == 0, "qea_facility_select: workspace must be 16-byte, x 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const FlWorkspace w = fl_carve(workspace, n);
  if (hipMemsetAsync(workspace, 0, qea_facility_workspace_bytes(n, d), s) != hipSuccess) {      // flag, M, cur = +0.0, picked
    qea_set_error("qea_facility_select: workspace memset failed");
    return QEA_ERR_LAUNCH;
  }
  fl_launch_pairs<FL_MAXDIST>(x, n, d, w, s);
  QEA_CHECK_LAUNCH();
  for (int t = 0; t < k; ++t) {
    fl_launch_pairs<FL_GAIN>(x, n, d, w, s);
    hipLaunchKernelGGL(fl_select_kernel, dim3(1), dim3(FL_SELECT_THREADS), 0, s, x, n, d, t, w.cur, w.gain, w.picked, w.flag, w.m_bits,
                       ranking_out, gain_out);
  }
  QEA_CHECK_LAUNCH();
  return QEA_OK;
}

extern "C" int qea_facility_status(const void* workspace, void* stream) {
  QEA_REQUIRE(workspace, "qea_facility_status: null workspace");
  int flag = 0;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(&flag, workspace, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    qea_set_error("qea_facility_status: reading the flag word failed: %s", hipGetErrorString(hipGetLastError()));
    return QEA_ERR_LAUNCH;
  }
  QEA_REQUIRE(!(flag & FL_FLAG_NONFINITE), "qea_facility_select: non-finite feature (NaN or inf) in x; no ranking was written");
  QEA_REQUIRE(!(flag & FL_FLAG_OVERFLOW), "qea_facility_select: a squared distance overflows fp64; no ranking was written");
  QEA_REQUIRE(!(flag & FL_FLAG_NO_WINNER), "qea_facility_select: a pick found no candidate (internal error)");
  return QEA_OK;
}
