// Sparse triangular solves on the pixel grid: forward_substitution, backward_substitution and
// inverse_diagonal of utils/triag_solve.py:76-115, 163-202 and utils/triag_solve/triag_solve_cuda.cu:72-139.  The operator
// couples a pixel to its left, upper and upper-left neighbour (lower form; the upper form is its mirror image):
//   (J y)[i,j] = A[i,j] y[i,j] + B[i,j-1] y[i,j-1] + C[i-1,j] y[i-1,j] + D[i-1,j-1] y[i-1,j-1]
// The reference runs the M*N recurrence in one thread per plane.  Here one wave owns a plane, one LANE owns a ROW, and the
// rows are skewed: at step t the lane of row r computes column t - r, so the wave walks the anti-diagonals.
//   left neighbour        the lane's own result of step t - 1
//   upper neighbour       the result of the lane above from step t - 1: one shift by one lane per step (DPP wave_shr:1)
//   upper-left neighbour  what the lane received one step earlier
// Rows beyond 64 are swept as further 64-row strips by the same wave; the last row of a strip stays in LDS (`bnd`) and
// enters lane 0 of the next strip through the `old` operand of the same shift.  The dependent chain per plane is
// ceil(M / 64) * (N + 63) steps of {shift, mul, sub, sub, sub, div} -- never M * N -- and holds no memory access:
//   * coefficients and right-hand side are staged in chunks of CW steps: a chunk is a 64 x CW PARALLELOGRAM of the grid
//     (row r needs columns t0 - r .. t0 + CW - 1 - r), fetched row segment by row segment (4 rows of 16 consecutive floats
//     per load instruction, where a skewed lane-per-row read would touch 64 cache lines), held in registers while the
//     previous chunk is computed, and then written to LDS tiles [row][step] of row stride CW + 1 (conflict-free for the
//     row-segment writes and for the lane-per-row reads);
//   * results go back through the same tiles (in place: a lane overwrites the operands it has consumed) and leave as row
//     segments as well.
// Cells outside the grid are staged as A = 1, B = C = D = X = 0 and so solve to exactly 0: the step loop has no
// predicate.  The order per element is the reference's (utils/triag_solve.py:86-92): subtract the rounded C, B and D
// products in turn, then a true division (-ffp-contract=off keeps the products unfused; the parts of the division that
// depend on A alone are scheduled off the chain by the compiler).  Every element's value is fixed by that order and
// independent of scheduling, so the solves and all five gradients are the bits of the reference's fp32 CPU run.  No
// atomics: the same bits in normal and deterministic mode.
//
// The backward of ForwardSubst / BackwardSubst is the same sweep over the opposite triangle with gY as right-hand side:
// when gX of a cell is computed, the gX of its three neighbours are in registers, which with the cell's own Y are all four
// coefficient gradients that belong to the cell (the coefficients it multiplied its neighbours with).
// inverse_diagonal runs the sweep once per source pixel (k,l) on the sub-grid of rows >= k and columns >= l (without D the
// solution is zero to the left of l) with a unit right-hand side, squares and sums in registers and stores one float.
#include "common.hpp"

namespace {

constexpr int NL = AF_WAVE;     // lanes = rows of a strip = threads of a workgroup
constexpr int CW = 16;          // steps per chunk
constexpr int TS = CW + 1;      // tile row stride, floats
constexpr int RPI = NL / CW;    // rows per staging instruction
constexpr int NIT = NL / RPI;   // staging instructions per tile
constexpr int MAX_M = 16384, MAX_N = 8192;  // bnd: (MAX_N + NL + CW) floats of LDS next to the tiles
enum { SOLVE = 0, BWD = 1, NORM = 2 };

// One plane, or the sub-grid of one that starts at `A`: logical cell (r, c) of the sweep is grid cell (r, c) for the lower
// form and (M-1-r, N-1-c) for the upper.
struct Plane {
  const float *A, *B, *C, *D, *X, *Y;  // X: right-hand side (NORM: unused); Y: the forward's solution (BWD only)
  float *oX, *gA, *gB, *gC, *gD;       // oX: the solution; g*: BWD only
  int M, N;                            // extent
  int sa, sb;                          // row strides of A / C / X / Y and of B / D
  int upper;
};

struct Cell {  // offsets of a logical cell's own element and of the coefficients that multiply its three neighbours
  bool in, hb, hc, hd;
  int ia, ib, ic, id;
};
__device__ __forceinline__ Cell cell_of(const Plane& g, int r, int c) {
  Cell q;
  q.in = r < g.M && c >= 0 && c < g.N;
  q.hb = q.in && c >= 1;
  q.hc = q.in && r >= 1;
  q.hd = q.hb && r >= 1;
  const int i = g.upper ? g.M - 1 - r : r, j = g.upper ? g.N - 1 - c : c;
  q.ia = i * g.sa + j;
  // lower: B[i][j-1], C[i-1][j], D[i-1][j-1] (utils/triag_solve.py:86-91); upper: B, C, D[i][j] (:107-112)
  q.ib = g.upper ? i * g.sb + j : i * g.sb + j - 1;
  q.ic = g.upper ? q.ia : q.ia - g.sa;
  q.id = g.upper ? q.ib : q.ib - g.sb;
  return q;
}

// lane l receives v of lane l - 1; lane 0 receives `first`
__device__ __forceinline__ float shift_up(float first, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf,
                                                    0xf, false));
}

// A phase change between the lanes' row-segment view and their own-row view of the tiles (a workgroup is one wave; every
// call site is in control flow that is uniform over it).
__device__ __forceinline__ void wave_sync() { __syncthreads(); }

template <int MODE>
struct Staged {  // one chunk in flight: NIT elements per lane and tile
  float a[NIT], b[NIT], c[NIT], d[NIT], x[NIT], y[MODE == BWD ? NIT : 1];
};

// the chunk of steps t0 .. t0 + CW - 1 of the strip that starts at row R0: global -> registers
template <int MODE>
__device__ __forceinline__ void fetch(const Plane& g, int R0, int t0, int lane, Staged<MODE>& s) {
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int rr = it * RPI + lane / CW, k = lane % CW;
    const int r = R0 + rr, c = t0 + k - rr;
    const Cell q = cell_of(g, r, c);
    s.a[it] = q.in ? g.A[q.ia] : 1.f;
    s.b[it] = q.hb ? g.B[q.ib] : 0.f;
    s.c[it] = q.hc ? g.C[q.ic] : 0.f;
    s.d[it] = (q.hd && g.D) ? g.D[q.id] : 0.f;
    if (MODE == NORM)
      s.x[it] = (r == 0 && c == 0) ? 1.f : 0.f;
    else
      s.x[it] = q.in ? g.X[q.ia] : 0.f;
    if (MODE == BWD) s.y[it] = q.in ? g.Y[q.ia] : 0.f;
  }
}

// registers -> tiles [row][step]
template <int MODE>
__device__ __forceinline__ void stage(const Staged<MODE>& s, int lane, float (*tile)[NL * TS]) {
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int o = (it * RPI + lane / CW) * TS + lane % CW;
    tile[0][o] = s.a[it];
    tile[1][o] = s.b[it];
    tile[2][o] = s.c[it];
    tile[3][o] = s.d[it];
    tile[4][o] = s.x[it];
    if (MODE == BWD) tile[5][o] = s.y[it];
  }
}

// tiles -> global as row segments; the strip's last row also goes to bnd for the strip below
template <int MODE>
__device__ __forceinline__ void drain(const Plane& g, int R0, int t0, int lane, float (*tile)[NL * TS], float* bnd) {
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int rr = it * RPI + lane / CW, k = lane % CW;
    const int c = t0 + k - rr, o = rr * TS + k;
    const Cell q = cell_of(g, R0 + rr, c);
    if (q.in) {
      const float v = tile[4][o];
      if (MODE != NORM) g.oX[q.ia] = v;
      if (rr == NL - 1) bnd[c] = v;
      if (MODE == BWD) g.gA[q.ia] = tile[0][o];
    }
    if (MODE == BWD) {
      if (q.hb) g.gB[q.ib] = tile[1][o];
      if (q.hc) g.gC[q.ic] = tile[2][o];
      if (q.hd && g.gD) g.gD[q.id] = tile[3][o];
    }
  }
}

// The whole sweep of one plane by one wave.  bnd: N + NL + CW floats.  Every loop bound depends on g.M and g.N alone
// (uniform over the wave: the DPP shift needs all 64 lanes active, and every thread reaches every barrier).  Returns the
// lane's sum of squares (NORM).
template <int MODE>
__device__ __forceinline__ float sweep(const Plane& g, float (*tile)[NL * TS], float* bnd) {
  const int lane = threadIdx.x;
  for (int i = lane; i < g.N + NL + CW; i += NL) bnd[i] = 0.f;  // no row above the first strip; columns >= N stay 0
  float acc = 0.f;
  Staged<MODE> s;
  for (int R0 = 0; R0 < g.M; R0 += NL) {
    const int rows = min(NL, g.M - R0);
    const int nchunk = (g.N + rows - 1 + CW - 1) / CW;  // steps of the strip: N + rows - 1
    const bool row_in = R0 + lane < g.M;
    fetch<MODE>(g, R0, 0, lane, s);
    wave_sync();  // after the previous strip's drain (tiles, bnd) and the zero fill
    stage<MODE>(s, lane, tile);
    wave_sync();
    float y = 0.f, ul = 0.f;  // the lane's previous result; the upper neighbour's result of two steps ago
    for (int ch = 0; ch < nchunk; ++ch) {
      const int t0 = ch * CW;
      if (ch + 1 < nchunk) fetch<MODE>(g, R0, t0 + CW, lane, s);  // in flight while this chunk is computed
      float va[CW], vb[CW], vc[CW], vd[CW], vx[CW], vy[CW], first[CW];
#pragma unroll
      for (int k = 0; k < CW; ++k) {
        const int o = lane * TS + k;
        va[k] = tile[0][o], vb[k] = tile[1][o], vc[k] = tile[2][o], vd[k] = tile[3][o], vx[k] = tile[4][o];
        if (MODE == BWD) vy[k] = tile[5][o];
        first[k] = bnd[t0 + k];  // row R0 - 1 at lane 0's column (the same address in every lane)
      }
#pragma unroll
      for (int k = 0; k < CW; ++k) {
        const float up = shift_up(first[k], y);
        float t = vx[k] - vc[k] * up;  // the reference's order and roundings
        t = t - vb[k] * y;
        t = t - vd[k] * ul;
        const float yn = t / va[k];
        if (MODE == BWD) {  // the gradients of the coefficients this cell multiplied its neighbours with
          const float ny = -vy[k];
          va[k] = yn * ny, vb[k] = y * ny, vc[k] = up * ny, vd[k] = ul * ny;
        }
        if (MODE == NORM) acc = row_in ? fmaf(yn, yn, acc) : acc;  // rows below the grid see the last row through zero coefficients
        vx[k] = yn;
        ul = up;
        y = yn;
      }
#pragma unroll
      for (int k = 0; k < CW; ++k) {
        const int o = lane * TS + k;
        tile[4][o] = vx[k];
        if (MODE == BWD) tile[0][o] = va[k], tile[1][o] = vb[k], tile[2][o] = vc[k], tile[3][o] = vd[k];
      }
      wave_sync();
      drain<MODE>(g, R0, t0, lane, tile, bnd);
      if (ch + 1 < nchunk) {
        wave_sync();
        stage<MODE>(s, lane, tile);
      }
      wave_sync();
    }
  }
  return acc;
}

__device__ __forceinline__ const float* at(const float* p, long off) { return p ? p + off : nullptr; }
__device__ __forceinline__ float* at(float* p, long off) { return p ? p + off : nullptr; }

// grid (P); MODE SOLVE: X -> oX; MODE BWD: X = gY, oX = gX, `upper` is the direction of THIS solve
template <int MODE>
__global__ __launch_bounds__(NL) void triag_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                   const float* __restrict__ C, const float* __restrict__ D,
                                                   const float* __restrict__ X, const float* __restrict__ Y,
                                                   float* __restrict__ oX, float* __restrict__ gA, float* __restrict__ gB,
                                                   float* __restrict__ gC, float* __restrict__ gD, int M, int N, int upper) {
  __shared__ float tile[MODE == BWD ? 6 : 5][NL * TS];
  extern __shared__ float bnd[];
  const long p = blockIdx.x;
  const long na = (long)M * N, nb = (long)M * (N - 1), nc = (long)(M - 1) * N, nd = (long)(M - 1) * (N - 1);
  Plane g;
  g.A = A + p * na, g.B = at(B, p * nb), g.C = at(C, p * nc), g.D = at(D, p * nd), g.X = X + p * na, g.Y = at(Y, p * na);
  g.oX = oX + p * na, g.gA = at(gA, p * na), g.gB = at(gB, p * nb), g.gC = at(gC, p * nc), g.gD = at(gD, p * nd);
  g.M = M, g.N = N, g.sa = N, g.sb = N - 1, g.upper = upper;
  sweep<MODE>(g, tile, bnd);
}

// grid (P * M * N): one wave per source pixel
__global__ __launch_bounds__(NL) void triag_invdiag_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                           const float* __restrict__ C, float* __restrict__ H, int M,
                                                           int N) {
  __shared__ float tile[5][NL * TS];
  extern __shared__ float bnd[];
  const long e = blockIdx.x;
  const long p = e / ((long)M * N);
  const int k = (int)(e % ((long)M * N)) / N, l = (int)(e % N);
  Plane g;
  g.A = A + p * M * N + (long)k * N + l;
  g.B = at(B, p * M * (N - 1) + (long)k * (N - 1) + l);
  g.C = at(C, p * (M - 1) * N + (long)k * N + l);
  g.D = nullptr, g.X = nullptr, g.Y = nullptr;
  g.oX = g.gA = g.gB = g.gC = g.gD = nullptr;
  g.M = M - k, g.N = N - l, g.sa = N, g.sb = N - 1, g.upper = 0;
  const float s = af_wave_sum(sweep<NORM>(g, tile, bnd));
  if (threadIdx.x == 0) H[e] = s;
}

inline int check_dims(long P, int M, int N) {
  AF_REQUIRE(P >= 1 && M >= 1 && N >= 1, ARFLOW_ESHAPE);
  AF_REQUIRE(P <= 0x7fffffffL && M <= MAX_M && N <= MAX_N, ARFLOW_ESHAPE);
  return ARFLOW_OK;
}
inline size_t bnd_bytes(int N) { return sizeof(float) * (size_t)(N + NL + CW); }

}  // namespace

extern "C" int arflow_triag_solve(const float* A, const float* B, const float* C, const float* D, const float* X, float* Y,
                                  int P, int M, int N, int upper, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(A);
  AF_REQUIRE_PTR(X);
  AF_REQUIRE_PTR(Y);
  if (N > 1) AF_REQUIRE_PTR(B);
  if (M > 1) AF_REQUIRE_PTR(C);
  const int rc = check_dims(P, M, N);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(upper == 0 || upper == 1, ARFLOW_EPARAM);
  if (M == 1 || N == 1) D = nullptr;  // no elements
  hipLaunchKernelGGL(triag_kernel<SOLVE>, dim3(P), dim3(NL), bnd_bytes(N), (hipStream_t)stream, A, B, C, D, X,
                     (const float*)nullptr, Y, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, M, N, upper);
  return af_launch_status();
}

extern "C" int arflow_triag_solve_bwd(const float* A, const float* B, const float* C, const float* D, const float* Y,
                                      const float* gY, float* gX, float* gA, float* gB, float* gC, float* gD, int P, int M,
                                      int N, int upper, arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(A);
  AF_REQUIRE_PTR(Y);
  AF_REQUIRE_PTR(gY);
  AF_REQUIRE_PTR(gX);
  AF_REQUIRE_PTR(gA);
  if (N > 1) {
    AF_REQUIRE_PTR(B);
    AF_REQUIRE_PTR(gB);
  }
  if (M > 1) {
    AF_REQUIRE_PTR(C);
    AF_REQUIRE_PTR(gC);
  }
  const int rc = check_dims(P, M, N);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE(upper == 0 || upper == 1, ARFLOW_EPARAM);
  if (M == 1 || N == 1) D = nullptr, gD = nullptr;
  if (D) AF_REQUIRE_PTR(gD);
  AF_REQUIRE(D || !gD, ARFLOW_EPARAM);
  // the transposed system: the opposite triangle with the same coefficient arrays (utils/triag_solve.py:175, :196)
  hipLaunchKernelGGL(triag_kernel<BWD>, dim3(P), dim3(NL), bnd_bytes(N), (hipStream_t)stream, A, B, C, D, gY, Y, gX, gA, gB,
                     gC, gD, M, N, 1 - upper);
  return af_launch_status();
}

extern "C" int arflow_triag_inverse_diagonal(const float* A, const float* B, const float* C, float* H, int P, int M, int N,
                                             arflow_stream_t stream) {
  af_clear_stale_error();
  AF_REQUIRE_PTR(A);
  AF_REQUIRE_PTR(H);
  if (N > 1) AF_REQUIRE_PTR(B);
  if (M > 1) AF_REQUIRE_PTR(C);
  const int rc = check_dims(P, M, N);
  if (rc != ARFLOW_OK) return rc;
  AF_REQUIRE((long)P * M * N <= 0x7fffffffL, ARFLOW_ESHAPE);  // one workgroup per source pixel
  hipLaunchKernelGGL(triag_invdiag_kernel, dim3((unsigned)((long)P * M * N)), dim3(NL), bnd_bytes(N), (hipStream_t)stream, A,
                     B, C, H, M, N);
  return af_launch_status();
}
