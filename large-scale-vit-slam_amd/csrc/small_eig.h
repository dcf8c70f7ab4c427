// The small fp64 solvers of the pose and Sim(3) kernels, run by one lane: the 3x3 symmetric
// eigen-decomposition and the SVD that Umeyama's closed form takes from it (irls_solve in align.hip,
// umeyama3 below for pose.hip and gt_points.hip), and the top eigenvector of a symmetric 4x4 (the Markley
// quaternion mean of pose_compose_kernel and pose_align_kernel, pose.hip).
//
// Plain C++ apart from the two qualifiers, so that a host program can define them away and run the
// very same code (tests/small_eig_host.cpp).
//
// The 3x3 and the 4x4 Jacobi are two routines on purpose: their stopping rules (sum |a_pq| <= 1e-18 sum
// |a_pp| against sum a_pq^2 < 1e-60) and their skip rules (== 0 against < 1e-300) differ, and either
// one given the other's rule would change result bits.
#pragma once
#include <math.h>

// ---- 3x3 symmetric eigen-decomposition (cyclic Jacobi, fp64): A -> diagonal, V's columns the vectors
static __device__ void jacobi3(double A[3][3], double V[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
    const double scale = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
    if (off <= 1e-300 || off <= 1e-18 * scale) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 3; ++k) {  // A = J^T A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

static __device__ __forceinline__ double det3(const double M[3][3]) {
  return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
         M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// The SVD Sg = U diag(sv) Vs^T of a 3x3 cross-covariance as Umeyama's closed form needs it, and
// det(U Vs^T): V from Jacobi on Sg^T Sg, singular values descending, u_k = Sg v_k / |Sg v_k| for the two
// largest, u_2 = u_0 x u_1, and v_2's sign chosen so that Sg v_2 = sv_2 u_2 with sv_2 >= 0 (a valid SVD
// pair).  det(U) is then +1, and d = sign(det(U Vs^T)) is the reference's det(u) det(v) < 0 test for any
// valid pair (d v_2 does not depend on v_2's sign).  What d is at a determinant of 0, the scale and the
// translation are the caller's.
static __device__ void svd3_for_umeyama(const double Sg[3][3], double U[3][3], double Vs[3][3], double sv[3],
                                        double* det_UVt) {
  double A[3][3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i][j] = Sg[0][i] * Sg[0][j] + Sg[1][i] * Sg[1][j] + Sg[2][i] * Sg[2][j];
  jacobi3(A, V);
  int ord[3] = {0, 1, 2};  // eigenvalues descending
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2 - i; ++j)
      if (A[ord[j]][ord[j]] < A[ord[j + 1]][ord[j + 1]]) {
        const int tmp = ord[j];
        ord[j] = ord[j + 1];
        ord[j + 1] = tmp;
      }
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i) Vs[i][k] = V[i][ord[k]];
  for (int k = 0; k < 2; ++k) {
    double u[3], nrm = 0.0;
    for (int i = 0; i < 3; ++i) {
      u[i] = Sg[i][0] * Vs[0][k] + Sg[i][1] * Vs[1][k] + Sg[i][2] * Vs[2][k];
      nrm += u[i] * u[i];
    }
    nrm = sqrt(nrm);
    sv[k] = nrm;
    for (int i = 0; i < 3; ++i) U[i][k] = nrm > 0 ? u[i] / nrm : (i == k ? 1.0 : 0.0);
  }
  // Rank <= 1 (collinear clouds or camera centres, two points): Sg v_1 is rounding noise and its
  // direction is not orthogonal to u_0.  In irls_solve every entry of Sg is a sum of fp64 products
  // reduced through at most ceil(n / 65536) + 6 + 4 + 256 additions (thread, wave, block, the NB
  // partials), so up to n = 2^24 it carries at most about 2^9 * 2^-53 = 2^-44 of
  // sum w |y_c| |x_c| / W <= sqrt(var_x var_y), which is sv_0 for a rank-1 cloud; v_1's own error adds
  // 2^-52 sv_0.  (gt_pose_align_kernel's sums are shorter: a lane's frames, then 64 lanes.)  Below
  // 2^-40 sv_0 (16 x that bound) sv_1 carries no information about the rotation round u_0, which the
  // data then does not determine: take any unit vector orthogonal to u_0, from the axis u_0 is
  // furthest from.
  if (sv[1] <= 0x1p-40 * sv[0]) {
    int j = 0;
    for (int i = 1; i < 3; ++i)
      if (fabs(U[i][0]) < fabs(U[j][0])) j = i;
    double nrm = 0.0;
    for (int i = 0; i < 3; ++i) {
      U[i][1] = (i == j ? 1.0 : 0.0) - U[j][0] * U[i][0];
      nrm += U[i][1] * U[i][1];
    }
    nrm = sqrt(nrm);
    for (int i = 0; i < 3; ++i) U[i][1] /= nrm;
  }
  U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
  U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
  U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  {
    double u[3];
    for (int i = 0; i < 3; ++i) u[i] = Sg[i][0] * Vs[0][2] + Sg[i][1] * Vs[1][2] + Sg[i][2] * Vs[2][2];
    const double proj = u[0] * U[0][2] + u[1] * U[1][2] + u[2] * U[2][2];
    if (proj < 0) {
      for (int i = 0; i < 3; ++i) Vs[i][2] = -Vs[i][2];
    }
    sv[2] = fabs(proj);
  }
  double UVt[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) UVt[i][j] = U[i][0] * Vs[j][0] + U[i][1] * Vs[j][1] + U[i][2] * Vs[j][2];
  *det_UVt = det3(UVt);
}

// Umeyama's closed form (alignment.py:6-59) from the centred cross-covariance Sg = E[(y - my)(x - mx)^T]
// and sigma_x = E|x - mx|^2: R = U diag(1, 1, d) V^T, c = tr(D diag(1, 1, d)) / sigma_x, on the SVD above
// (gt_pose_align_kernel in pose.hip, gp_solve_kernel in gt_points.hip; not every includer calls it).
[[maybe_unused]] static __device__ void umeyama3(const double Sg[3][3], double sigma_x, double R[3][3], double* c_out) {
  double U[3][3], Vs[3][3], sv[3], det;
  svd3_for_umeyama(Sg, U, Vs, sv, &det);
  const double d = det < 0 ? -1.0 : 1.0;  // the reflection fix (:39-40)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = U[i][0] * Vs[j][0] + U[i][1] * Vs[j][1] + d * U[i][2] * Vs[j][2];
  *c_out = (sv[0] + sv[1] + d * sv[2]) / sigma_x;  // sigma_x == 0: inf or NaN, as the reference's 1 / sigma_x
}

// Largest-eigenvalue unit eigenvector of a symmetric 4x4 (cyclic Jacobi, fp64).  The winning column is
// picked by selects: V[k][b] with a run-time b would put V into scratch memory.
static __device__ void top_eigvec4(const double Min[4][4], double* v) {
  double A[4][4], V[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      A[i][j] = Min[i][j];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 32; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 4; ++p)
      for (int q = p + 1; q < 4; ++q) off += A[p][q] * A[p][q];
    if (off < 1e-60) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        if (fabs(A[p][q]) < 1e-300) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {  // A <- J^T A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int b = 0;
  double best = A[0][0];
  for (int i = 1; i < 4; ++i)
    if (A[i][i] > best) { best = A[i][i]; b = i; }
  double col[4];
  for (int k = 0; k < 4; ++k) col[k] = b == 0 ? V[k][0] : b == 1 ? V[k][1] : b == 2 ? V[k][2] : V[k][3];
  double n = 0.0;
  for (int k = 0; k < 4; ++k) n += col[k] * col[k];
  n = sqrt(n);
  for (int k = 0; k < 4; ++k) v[k] = col[k] / n;
}
