// k_small_svd.hpp - the small-matrix routines of the geometry entries: what cv::SVD, cv::eigen, cv::Mat::inv, cv::determinant and cv::gemm do
// on 4x4, 16x9, 8x9 and 3x3 binary32 matrices in KannalaBrandt8::Triangulate, LocalMapping's and TwoViewReconstruction's Triangulate,
// ComputeH21 / ComputeF21 / ReconstructH / DecomposeE and Sim3Solver::ComputeSim3.  cv::SVD is OpenCV's own Jacobi or LAPACK's sgesdd, by its
// build: these routines are the PROJECT'S definition ("parity unpinned"), ONE one-sided (Hestenes) Jacobi iteration in
// binary32 with the constants below, and EVERY Jacobi routine of the library lives here:
//   jacobiAngle     the rotation of one column pair from a = |ci|^2, b = |cj|^2, p = ci.cj, stated once for every routine below;
//   jacobiPair<N>   one pair of a sweep on columns of N floats in registers.  The three register routines below call it pair by pair, in
//                   the order (i, j), i < j, until a sweep rotates nothing or kJacobiSweeps sweeps are done.  That driver is WRITTEN OUT
//                   three times on purpose: as one template every 4-column kernel took 65 more VGPRs (docs/history/r30_small_math.md);
//   nullVector4     vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on a 4x4 matrix: the column of smallest squared norm
//                   selects V's column, then one correction step in binary64 (tests/triangulation_two_eyes_walk.py states it too);
//   topEigenvector4 cv::eigen's row 0 on a symmetric 4x4 matrix (Sim3Solver's quaternion; k_sim3_solver.hpp says why it is shifted);
//   nullVector9<M>  vt.row(8) of an M x 9 matrix (M = 16: ComputeH21, M = 8: ComputeF21, rank <= 8: one column goes to zero).  The matrix,
//                   its copy and V live in MEMORY (LDS on the device, one lane works on them): nothing is indexed at run time in registers.
//                   Pair order of a sweep: (i, j) for i = 0 .. 7, j = i + 1 .. 8; every dot product runs over the rows k = 0 .. M - 1 in
//                   order.  The column of smallest squared norm selects V's column, of equal norms the highest index; then nullVector4's one
//                   correction step against the ORIGINAL matrix in binary64.  nullVector9Wave<M> is the same definition with the rows over the
//                   lanes of a wave (device only): registers instead of memory, every sum a chain over the lanes in row order;
//   svd3            the full SVD A = U diag(w) Vt of a 3x3 matrix with w descending (ComputeF21's rank-2 step, ReconstructH, DecomposeE):
//                   the same iteration on the three columns in registers, pair order (0,1) (0,2) (1,2); w[i] = sqrt of the squared norm
//                   (float sum, left to right), ordered descending (of equal values the lower column first); U's first two columns are the
//                   rotated columns divided by w, its THIRD is cross(u0, u1), negated when it points against the third rotated column -
//                   so a rank-2 matrix (an essential matrix) has a well-defined u.col(2) and U diag(w) Vt is A in every case;
//   det3, inv3      cv::determinant and cv::Mat::inv (DECOMP_LU) on a 3x3 float matrix as OpenCV 3.4 writes them out: the cofactor expansion
//                   in binary64 from the float elements, inv = float(cofactor * (1 / det)), the zero matrix when det == 0;
//   gemm3           a 3x3 * 3x3 product, one gemmRow per element with a scale (k_match_helpers.hpp).
// The sign and order freedom of an SVD is fixed by the above and may differ from OpenCV's: in ReconstructH and DecomposeE it can permute
// the 8 or 4 motion hypotheses, never change their set.
// Takes sqrtFloat32 from k_small_math.hpp, gemmRow from k_match_helpers.hpp, ORBX_LDS from k_lds_vec.hpp; nothing from a feature header.
// Plain arithmetic only: compiles for the host behind tests/cpp/host_shim.
#pragma once
#include "k_lds_vec.hpp"
#include "k_match_helpers.hpp"
#include "k_small_math.hpp"

namespace orbx {

// ---- the iteration's constants (DESIGN.md section 2 quotes them) ----
constexpr int kJacobiSweeps = 15;                    // cap on sweeps: the bound that ends a NaN or degenerate matrix
constexpr float kJacobiEps = 0x1p-22f;               // a pair rotates when |p| > kJacobiEps * sqrt(a * b)  (2 * FLT_EPSILON)
constexpr float kJacobiPolishRatio = 64.0f;          // the correction step uses the columns whose squared norm exceeds this times the smallest

// whether the pair rotates, and by which (c, s)
__device__ __forceinline__ bool jacobiAngle(float a, float b, float p, float& c, float& s) {
    if (!(fabsf(p) > __fmul_rn(kJacobiEps, sqrtFloat32(__fmul_rn(a, b))))) return false;      // (a NaN never rotates)
    p = __fmul_rn(p, 2.0f);
    const float beta = __fsub_rn(a, b), gamma = sqrtFloat32(__fadd_rn(__fmul_rn(p, p), __fmul_rn(beta, beta)));
    // beta < 0: s = sqrt(((gamma - beta) * 0.5) / gamma), c = p / (gamma * s * 2); else c = sqrt((gamma + beta) / (gamma * 2)), s = p / (gamma * c * 2)
    const bool swap = beta < 0.0f;
    const float root = swap ? sqrtFloat32(__fdiv_rn(__fmul_rn(__fsub_rn(gamma, beta), 0.5f), gamma))
                            : sqrtFloat32(__fdiv_rn(__fadd_rn(gamma, beta), __fmul_rn(gamma, 2.0f)));
    const float other = __fdiv_rn(p, __fmul_rn(__fmul_rn(gamma, root), 2.0f));
    c = swap ? other : root;
    s = swap ? root : other;
    return true;
}

// one pair of a sweep: columns i and j of the working matrix and of V, N floats each in registers
template <int N>
__device__ __forceinline__ void jacobiPair(float (&ai)[N], float (&aj)[N], float (&vi)[N], float (&vj)[N], bool& rotated) {
    float a = 0.0f, b = 0.0f, p = 0.0f;
#pragma unroll
    for (int k = 0; k < N; k++) {
        a = __fadd_rn(a, __fmul_rn(ai[k], ai[k]));
        b = __fadd_rn(b, __fmul_rn(aj[k], aj[k]));
        p = __fadd_rn(p, __fmul_rn(ai[k], aj[k]));
    }
    float c, s;
    if (!jacobiAngle(a, b, p, c, s)) return;
    rotated = true;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const float x0 = ai[k], x1 = aj[k], y0 = vi[k], y1 = vj[k];
        ai[k] = __fadd_rn(__fmul_rn(c, x0), __fmul_rn(s, x1));
        aj[k] = __fsub_rn(__fmul_rn(c, x1), __fmul_rn(s, x0));
        vi[k] = __fadd_rn(__fmul_rn(c, y0), __fmul_rn(s, y1));
        vj[k] = __fsub_rn(__fmul_rn(c, y1), __fmul_rn(s, y0));
    }
}

// The right singular vector of A's smallest singular value.  A is row-major; out is NOT normalised in sign (it cancels in x / w).
// The column of smallest squared norm selects V's column, of equal norms the highest index (a NaN norm never wins: column 3).
__device__ __forceinline__ void nullVector4(const float (&A)[16], float (&out)[4]) {
    float c0[4], c1[4], c2[4], c3[4];
    float v0[4] = {1.f, 0.f, 0.f, 0.f}, v1[4] = {0.f, 1.f, 0.f, 0.f}, v2[4] = {0.f, 0.f, 1.f, 0.f}, v3[4] = {0.f, 0.f, 0.f, 1.f};
#pragma unroll
    for (int r = 0; r < 4; r++) { c0[r] = A[4 * r]; c1[r] = A[4 * r + 1]; c2[r] = A[4 * r + 2]; c3[r] = A[4 * r + 3]; }
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        bool rotated = false;
        jacobiPair<4>(c0, c1, v0, v1, rotated);
        jacobiPair<4>(c0, c2, v0, v2, rotated);
        jacobiPair<4>(c0, c3, v0, v3, rotated);
        jacobiPair<4>(c1, c2, v1, v2, rotated);
        jacobiPair<4>(c1, c3, v1, v3, rotated);
        jacobiPair<4>(c2, c3, v2, v3, rotated);
        if (!rotated) break;
    }
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        n0 = __fadd_rn(n0, __fmul_rn(c0[k], c0[k])); n1 = __fadd_rn(n1, __fmul_rn(c1[k], c1[k]));
        n2 = __fadd_rn(n2, __fmul_rn(c2[k], c2[k])); n3 = __fadd_rn(n3, __fmul_rn(c3[k], c3[k]));
    }
    int sel = 3;
    float best = n3;
    if (n2 < best) { best = n2; sel = 2; }
    if (n1 < best) { best = n1; sel = 1; }
    if (n0 < best) { best = n0; sel = 0; }
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = sel == 0 ? v0[k] : sel == 1 ? v1[k] : sel == 2 ? v2[k] : v3[k];
    // One correction step.  The rotations' roundings leave `out` with a component eps_i along each other column v_i of V; A*out, accumulated
    // in binary64 from the ORIGINAL matrix, shows it: the rotated column c_i is sigma_i*u_i, so eps_i = (c_i . A*out) / |c_i|^2.  Taken only
    // against columns whose squared norm is above kJacobiPolishRatio times the selected one (a column as small as the selected one spans
    // the same null space, and its c_i is rounding noise).
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double acc = __dmul_rn((double)A[4 * k], (double)out[0]);
#pragma unroll
        for (int c = 1; c < 4; c++) acc = __dadd_rn(acc, __dmul_rn((double)A[4 * k + c], (double)out[c]));
        r[k] = acc;
    }
    auto component = [&](const float (&c)[4], float n) {
        double acc = __dmul_rn((double)c[0], r[0]);
#pragma unroll
        for (int k = 1; k < 4; k++) acc = __dadd_rn(acc, __dmul_rn((double)c[k], r[k]));
        return __fdiv_rn((float)acc, n);
    };
    const float bound = __fmul_rn(kJacobiPolishRatio, best);
    const float e0 = sel != 0 && n0 > bound ? component(c0, n0) : 0.0f, e1 = sel != 1 && n1 > bound ? component(c1, n1) : 0.0f,
                e2 = sel != 2 && n2 > bound ? component(c2, n2) : 0.0f, e3 = sel != 3 && n3 > bound ? component(c3, n3) : 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++)
        out[k] = __fsub_rn(__fsub_rn(__fsub_rn(__fsub_rn(out[k], __fmul_rn(e0, v0[k])), __fmul_rn(e1, v1[k])), __fmul_rn(e2, v2[k])), __fmul_rn(e3, v3[k]));
}

// The eigenvector of the largest eigenvalue of the symmetric 4x4 Nm (row-major), sign fixed.  The iteration runs on Nm + mu * I, mu = the
// Frobenius norm of Nm (a float sum of float squares, left to right): the column of LARGEST squared norm selects V's column, of equal norms
// the lowest index; the first component that is not zero is made positive.
__device__ __forceinline__ void topEigenvector4(const float (&Nm)[16], float (&q)[4]) {
    float fro = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; k++) fro = __fadd_rn(fro, __fmul_rn(Nm[k], Nm[k]));
    const float mu = sqrtFloat32(fro);
    float c0[4], c1[4], c2[4], c3[4], v0[4] = {1.f, 0.f, 0.f, 0.f}, v1[4] = {0.f, 1.f, 0.f, 0.f}, v2[4] = {0.f, 0.f, 1.f, 0.f}, v3[4] = {0.f, 0.f, 0.f, 1.f};
#pragma unroll
    for (int r = 0; r < 4; r++) { c0[r] = Nm[4 * r]; c1[r] = Nm[4 * r + 1]; c2[r] = Nm[4 * r + 2]; c3[r] = Nm[4 * r + 3]; }
    c0[0] = __fadd_rn(c0[0], mu); c1[1] = __fadd_rn(c1[1], mu); c2[2] = __fadd_rn(c2[2], mu); c3[3] = __fadd_rn(c3[3], mu);
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        bool rotated = false;
        jacobiPair<4>(c0, c1, v0, v1, rotated);
        jacobiPair<4>(c0, c2, v0, v2, rotated);
        jacobiPair<4>(c0, c3, v0, v3, rotated);
        jacobiPair<4>(c1, c2, v1, v2, rotated);
        jacobiPair<4>(c1, c3, v1, v3, rotated);
        jacobiPair<4>(c2, c3, v2, v3, rotated);
        if (!rotated) break;
    }
    auto norm2 = [](const float (&c)[4]) {
        return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c[0], c[0]), __fmul_rn(c[1], c[1])), __fmul_rn(c[2], c[2])), __fmul_rn(c[3], c[3]));
    };
    const float n0 = norm2(c0), n1 = norm2(c1), n2 = norm2(c2), n3 = norm2(c3);
    float best = n0;
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = v0[k];
    if (n1 > best) { best = n1; for (int k = 0; k < 4; k++) q[k] = v1[k]; }
    if (n2 > best) { best = n2; for (int k = 0; k < 4; k++) q[k] = v2[k]; }
    if (n3 > best) { best = n3; for (int k = 0; k < 4; k++) q[k] = v3[k]; }
    const bool neg = q[0] != 0.0f ? q[0] < 0.0f : q[1] != 0.0f ? q[1] < 0.0f : q[2] != 0.0f ? q[2] < 0.0f : q[3] < 0.0f;
    if (neg)
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = -q[k];
}

// W: the M x 9 matrix, row-major, overwritten by the rotated columns; A0: its untouched copy; V: 9 x 9 scratch.
template <int M>
__device__ __forceinline__ void nullVector9(ORBX_LDS float* W, const ORBX_LDS float* A0, ORBX_LDS float* V, float (&out)[9]) {
    for (int k = 0; k < 81; k++) V[k] = (k / 9 == k % 9) ? 1.0f : 0.0f;
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        bool rotated = false;
        for (int i = 0; i < 8; i++)
            for (int j = i + 1; j < 9; j++) {
                float a = 0.0f, b = 0.0f, p = 0.0f;
#pragma unroll
                for (int k = 0; k < M; k++) {
                    const float x0 = W[9 * k + i], x1 = W[9 * k + j];
                    a = __fadd_rn(a, __fmul_rn(x0, x0));
                    b = __fadd_rn(b, __fmul_rn(x1, x1));
                    p = __fadd_rn(p, __fmul_rn(x0, x1));
                }
                float c, s;
                if (!jacobiAngle(a, b, p, c, s)) continue;
                rotated = true;
#pragma unroll
                for (int k = 0; k < M; k++) {
                    const float x0 = W[9 * k + i], x1 = W[9 * k + j];
                    W[9 * k + i] = __fadd_rn(__fmul_rn(c, x0), __fmul_rn(s, x1));
                    W[9 * k + j] = __fsub_rn(__fmul_rn(c, x1), __fmul_rn(s, x0));
                }
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    const float y0 = V[9 * k + i], y1 = V[9 * k + j];
                    V[9 * k + i] = __fadd_rn(__fmul_rn(c, y0), __fmul_rn(s, y1));
                    V[9 * k + j] = __fsub_rn(__fmul_rn(c, y1), __fmul_rn(s, y0));
                }
            }
        if (!rotated) break;
    }
    float n[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < M; k++) a = __fadd_rn(a, __fmul_rn(W[9 * k + i], W[9 * k + i]));
        n[i] = a;
    }
    int sel = 8;
    float best = n[8];
#pragma unroll
    for (int i = 7; i >= 0; i--)
        if (n[i] < best) { best = n[i]; sel = i; }
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = V[9 * k + sel];
    // the correction step of nullVector4: r = A0 * out in binary64, its component along every rotated column well above the selected one
    double r[M];
#pragma unroll
    for (int k = 0; k < M; k++) {
        double acc = __dmul_rn((double)A0[9 * k], (double)out[0]);
#pragma unroll
        for (int c = 1; c < 9; c++) acc = __dadd_rn(acc, __dmul_rn((double)A0[9 * k + c], (double)out[c]));
        r[k] = acc;
    }
    const float bound = __fmul_rn(kJacobiPolishRatio, best);
    float e[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        double acc = __dmul_rn((double)W[i], r[0]);
#pragma unroll
        for (int k = 1; k < M; k++) acc = __dadd_rn(acc, __dmul_rn((double)W[9 * k + i], r[k]));
        e[i] = (i != sel && n[i] > bound) ? __fdiv_rn((float)acc, n[i]) : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        float o = out[k];
#pragma unroll
        for (int i = 0; i < 9; i++) o = __fsub_rn(o, __fmul_rn(e[i], V[9 * k + i]));
        out[k] = o;
    }
}

#if !defined(ORBX_HOST_ROW) && defined(__HIPCC__)
// ---- nullVector9 with the ROWS OVER THE LANES of a wave: the same definition, bit for bit ---------------------------------------------
// Lane k < M holds row k of the matrix (w), of its copy (a0) and, for k < 9, row k of V (v), all in registers; lanes from M on hold zeros.
// A dot product over the rows is the SAME left-to-right sum: one chain of v_readlane + v_add over lanes 0 .. M - 1, uniform on every lane
// (laneChain), so the angles are uniform and each lane rotates its own row.  No LDS, no barrier; the pair loops are unrolled (36 pairs), the
// column indices are constants.
template <int M>
__device__ __forceinline__ float laneChain(float x) {
    float s = 0.0f;
#pragma unroll
    for (int l = 0; l < M; l++) s = __fadd_rn(s, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)));
    return s;
}
__device__ __forceinline__ double readLaneDouble(double x, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
template <int M>
__device__ __forceinline__ void nullVector9Wave(const float (&a0)[9], float (&out)[9]) {
    const int lane = (int)threadIdx.x;
    float w[9], v[9];
#pragma unroll
    for (int c = 0; c < 9; c++) { w[c] = a0[c]; v[c] = lane == c ? 1.0f : 0.0f; }
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int j = i + 1; j < 9; j++) {
                const float x0 = w[i], x1 = w[j];
                const float a = laneChain<M>(__fmul_rn(x0, x0)), b = laneChain<M>(__fmul_rn(x1, x1)), p = laneChain<M>(__fmul_rn(x0, x1));
                float c, s;
                if (jacobiAngle(a, b, p, c, s)) {                                             // (uniform)
                    rotated = true;
                    const float y0 = v[i], y1 = v[j];
                    w[i] = __fadd_rn(__fmul_rn(c, x0), __fmul_rn(s, x1)); w[j] = __fsub_rn(__fmul_rn(c, x1), __fmul_rn(s, x0));
                    v[i] = __fadd_rn(__fmul_rn(c, y0), __fmul_rn(s, y1)); v[j] = __fsub_rn(__fmul_rn(c, y1), __fmul_rn(s, y0));
                }
            }
        if (!rotated) break;
    }
    float n[9];
#pragma unroll
    for (int i = 0; i < 9; i++) n[i] = laneChain<M>(__fmul_rn(w[i], w[i]));
    int sel = 8;
    float best = n[8];
#pragma unroll
    for (int i = 7; i >= 0; i--)
        if (n[i] < best) { best = n[i]; sel = i; }
    float own = v[8];                                                                         // V[lane][sel]
#pragma unroll
    for (int i = 0; i < 8; i++) own = sel == i ? v[i] : own;
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(own), k));
    double r = __dmul_rn((double)a0[0], (double)out[0]);                                      // row `lane` of A0 * out
#pragma unroll
    for (int c = 1; c < 9; c++) r = __dadd_rn(r, __dmul_rn((double)a0[c], (double)out[c]));
    const float bound = __fmul_rn(kJacobiPolishRatio, best);
    float o = own;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double prod = __dmul_rn((double)w[i], r);
        double acc = readLaneDouble(prod, 0);
#pragma unroll
        for (int k = 1; k < M; k++) acc = __dadd_rn(acc, readLaneDouble(prod, k));
        const float e = (i != sel && n[i] > bound) ? __fdiv_rn((float)acc, n[i]) : 0.0f;
        o = __fsub_rn(o, __fmul_rn(e, v[i]));
    }
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(o), k));
}
#endif

__device__ __forceinline__ void svd3Swap(float (&a)[3], float (&b)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) { const float t = a[k]; a[k] = b[k]; b[k] = t; }
}

// A = U diag(w) Vt, all row-major
__device__ __forceinline__ void svd3(const float (&A)[9], float (&U)[9], float (&w)[3], float (&Vt)[9]) {
    float c0[3], c1[3], c2[3], v0[3] = {1.f, 0.f, 0.f}, v1[3] = {0.f, 1.f, 0.f}, v2[3] = {0.f, 0.f, 1.f};
#pragma unroll
    for (int r = 0; r < 3; r++) { c0[r] = A[3 * r]; c1[r] = A[3 * r + 1]; c2[r] = A[3 * r + 2]; }
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        bool rotated = false;
        jacobiPair<3>(c0, c1, v0, v1, rotated);
        jacobiPair<3>(c0, c2, v0, v2, rotated);
        jacobiPair<3>(c1, c2, v1, v2, rotated);
        if (!rotated) break;
    }
    auto norm = [](const float (&c)[3]) { return sqrtFloat32(__fadd_rn(__fadd_rn(__fmul_rn(c[0], c[0]), __fmul_rn(c[1], c[1])), __fmul_rn(c[2], c[2]))); };
    float w0 = norm(c0), w1 = norm(c1), w2 = norm(c2);
    // descending, of equal values the lower column first (a bubble of three compares; a NaN stays where it is)
    auto order = [](float& wa, float& wb, float (&ca)[3], float (&cb)[3], float (&va)[3], float (&vb)[3]) {
        if (wb > wa) { const float t = wa; wa = wb; wb = t; svd3Swap(ca, cb); svd3Swap(va, vb); }
    };
    order(w0, w1, c0, c1, v0, v1);
    order(w1, w2, c1, c2, v1, v2);
    order(w0, w1, c0, c1, v0, v1);
    w[0] = w0; w[1] = w1; w[2] = w2;
    float u0[3], u1[3], u2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { u0[k] = __fdiv_rn(c0[k], w0); u1[k] = __fdiv_rn(c1[k], w1); }
    u2[0] = __fsub_rn(__fmul_rn(u0[1], u1[2]), __fmul_rn(u0[2], u1[1]));
    u2[1] = __fsub_rn(__fmul_rn(u0[2], u1[0]), __fmul_rn(u0[0], u1[2]));
    u2[2] = __fsub_rn(__fmul_rn(u0[0], u1[1]), __fmul_rn(u0[1], u1[0]));
    const float along = __fadd_rn(__fadd_rn(__fmul_rn(u2[0], c2[0]), __fmul_rn(u2[1], c2[1])), __fmul_rn(u2[2], c2[2]));
    if (along < 0.0f) { u2[0] = -u2[0]; u2[1] = -u2[1]; u2[2] = -u2[2]; }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        U[3 * k] = u0[k]; U[3 * k + 1] = u1[k]; U[3 * k + 2] = u2[k];
        Vt[k] = v0[k]; Vt[3 + k] = v1[k]; Vt[6 + k] = v2[k];
    }
}

__device__ __forceinline__ double det3(const float (&m)[9]) {
    auto minor2 = [](float a, float b, float c, float d) { return __dsub_rn(__dmul_rn((double)a, (double)b), __dmul_rn((double)c, (double)d)); };
    const double t0 = __dmul_rn((double)m[0], minor2(m[4], m[8], m[5], m[7])), t1 = __dmul_rn((double)m[1], minor2(m[3], m[8], m[5], m[6])),
                 t2 = __dmul_rn((double)m[2], minor2(m[3], m[7], m[4], m[6]));
    return __dadd_rn(__dsub_rn(t0, t1), t2);
}

__device__ __forceinline__ void inv3(const float (&m)[9], float (&out)[9]) {
    auto minor2 = [](float a, float b, float c, float d) { return __dsub_rn(__dmul_rn((double)a, (double)b), __dmul_rn((double)c, (double)d)); };
    double d = det3(m);
    if (d == 0.0) {
#pragma unroll
        for (int k = 0; k < 9; k++) out[k] = 0.0f;
        return;
    }
    d = __ddiv_rn(1.0, d);
    out[0] = (float)__dmul_rn(minor2(m[4], m[8], m[5], m[7]), d);
    out[1] = (float)__dmul_rn(minor2(m[2], m[7], m[1], m[8]), d);
    out[2] = (float)__dmul_rn(minor2(m[1], m[5], m[2], m[4]), d);
    out[3] = (float)__dmul_rn(minor2(m[5], m[6], m[3], m[8]), d);
    out[4] = (float)__dmul_rn(minor2(m[0], m[8], m[2], m[6]), d);
    out[5] = (float)__dmul_rn(minor2(m[2], m[3], m[0], m[5]), d);
    out[6] = (float)__dmul_rn(minor2(m[3], m[7], m[4], m[6]), d);
    out[7] = (float)__dmul_rn(minor2(m[1], m[6], m[0], m[7]), d);
    out[8] = (float)__dmul_rn(minor2(m[0], m[4], m[1], m[3]), d);
}

// out = alpha * A * B
__device__ __forceinline__ void gemm3(const float (&A)[9], const float (&B)[9], double alpha, float (&out)[9]) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float col[3] = {B[c], B[3 + c], B[6 + c]};
            out[3 * r + c] = gemmRow(A[3 * r], A[3 * r + 1], A[3 * r + 2], col, alpha, 0.f, false);
        }
}

}  // namespace orbx
