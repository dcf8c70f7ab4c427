// The solvers of csrc/small_eig.h on the host: the header is plain C++ once its two qualifiers are defined away,
// so the code the kernels run is compiled here with the host compiler (test_small_eig_host.py adds
// -fsanitize=address,undefined) and checked in fp64 on a fixed list:
//   3x3 Sg: identity, a diagonal with a repeated value, rank 1, a reflection (det(U Vs^T) < 0), ten seeded random
//     svd3_for_umeyama  |Sg - U diag(sv) Vs^T|_F <= 1e-12 |Sg|_F, sv descending and >= 0, det(U) = +1, the sign of
//                       det(U Vs^T) the sign of det(Sg)
//     jacobi3           on Sg^T Sg and on (Sg + Sg^T) / 2: |A v - lambda v|_2 <= 1e-12 |A|_F for the three pairs
//   4x4 symmetric: identity, a diagonal with a repeated top value, rank 1 (q q^T), ten seeded random
//     top_eigvec4       |v| = 1, |A v - lambda v|_2 <= 1e-12 |A|_F with lambda = v^T A v, and lambda >= every
//                       diagonal entry (the top of the spectrum bounds them)
// Exit status 0 and "small_eig_host: ok" when every check holds; each failure is printed.
#include <stdio.h>

#define __device__
#define __forceinline__ inline
#include "../large-scale-vit-slam_amd/csrc/small_eig.h"

static int failures = 0;

static void check(bool ok, const char* what, const char* name, double got, double bound) {
  if (ok) return;
  ++failures;
  printf("FAIL %s [%s]: %.3e against %.3e\n", what, name, got, bound);
}

// a fixed 64-bit LCG (Knuth's MMIX constants): uniform in [-1, 1)
static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(rng_state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

static double frob3(const double M[3][3]) {
  double s = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) s += M[i][j] * M[i][j];
  return sqrt(s);
}

static void check_jacobi3(const double A0[3][3], const char* name) {
  double A[3][3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i][j] = A0[i][j];
  jacobi3(A, V);
  const double scale = frob3(A0);
  for (int k = 0; k < 3; ++k) {
    double r = 0.0;
    for (int i = 0; i < 3; ++i) {
      const double e = A0[i][0] * V[0][k] + A0[i][1] * V[1][k] + A0[i][2] * V[2][k] - A[k][k] * V[i][k];
      r += e * e;
    }
    check(sqrt(r) <= 1e-12 * scale, "jacobi3 |A v - lambda v|", name, sqrt(r), 1e-12 * scale);
  }
}

static void check_svd3(const double Sg[3][3], const char* name) {
  double U[3][3], Vs[3][3], sv[3], det;
  svd3_for_umeyama(Sg, U, Vs, sv, &det);
  const double scale = frob3(Sg);
  double r = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double e = Sg[i][j] - (U[i][0] * sv[0] * Vs[j][0] + U[i][1] * sv[1] * Vs[j][1] + U[i][2] * sv[2] * Vs[j][2]);
      r += e * e;
    }
  check(sqrt(r) <= 1e-12 * scale, "svd3 |Sg - U diag(sv) Vs^T|", name, sqrt(r), 1e-12 * scale);
  check(sv[0] >= sv[1] && sv[2] >= 0.0, "svd3 order of sv", name, sv[1], sv[0]);
  check(fabs(det3(U) - 1.0) <= 1e-12, "svd3 det(U) - 1", name, fabs(det3(U) - 1.0), 1e-12);
  const double ds = det3(Sg);
  if (fabs(ds) > 1e-9 * scale * scale * scale)  // a full-rank Sg: the sign of det(U Vs^T) is that of det(Sg)
    check((det < 0) == (ds < 0) && fabs(fabs(det) - 1.0) <= 1e-12, "svd3 det(U Vs^T)", name, det, ds);
  double A[3][3], S[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      A[i][j] = Sg[0][i] * Sg[0][j] + Sg[1][i] * Sg[1][j] + Sg[2][i] * Sg[2][j];
      S[i][j] = 0.5 * (Sg[i][j] + Sg[j][i]);
    }
  check_jacobi3(A, name);
  check_jacobi3(S, name);
}

static void check_eig4(const double A[4][4], const char* name) {
  double v[4];
  top_eigvec4(A, v);
  double scale = 0.0, n = 0.0, lambda = 0.0, Av[4];
  for (int i = 0; i < 4; ++i) {
    Av[i] = 0.0;
    for (int j = 0; j < 4; ++j) {
      scale += A[i][j] * A[i][j];
      Av[i] += A[i][j] * v[j];
    }
    n += v[i] * v[i];
  }
  scale = sqrt(scale);
  for (int i = 0; i < 4; ++i) lambda += v[i] * Av[i];
  double r = 0.0;
  for (int i = 0; i < 4; ++i) r += (Av[i] - lambda * v[i]) * (Av[i] - lambda * v[i]);
  check(fabs(n - 1.0) <= 1e-12, "top_eigvec4 |v|^2 - 1", name, fabs(n - 1.0), 1e-12);
  check(sqrt(r) <= 1e-12 * scale, "top_eigvec4 |A v - lambda v|", name, sqrt(r), 1e-12 * scale);
  for (int i = 0; i < 4; ++i)
    check(lambda >= A[i][i] - 1e-12 * scale, "top_eigvec4 lambda below a diagonal entry", name, lambda, A[i][i]);
}

int main() {
  const double identity[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const double repeated[3][3] = {{2, 0, 0}, {0, 2, 0}, {0, 0, 0.5}};
  double rank1[3][3], reflection[3][3];
  const double a[3] = {0.48, -0.6, 0.64}, b[3] = {2.0, 1.0, -2.0};
  // a rotation by 0.7 rad about z after the mirror z -> -z, scaled: det < 0
  const double cz = cos(0.7), sz = sin(0.7);
  const double refl[3][3] = {{1.3 * cz, -1.3 * sz, 0}, {1.3 * sz, 1.3 * cz, 0}, {0, 0, -0.4}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      rank1[i][j] = a[i] * b[j];
      reflection[i][j] = refl[i][j];
    }
  check_svd3(identity, "identity");
  check_svd3(repeated, "repeated");
  check_svd3(rank1, "rank1");
  check_svd3(reflection, "reflection");
  {
    double U[3][3], Vs[3][3], sv[3], det;
    svd3_for_umeyama(reflection, U, Vs, sv, &det);
    check(det < 0, "svd3 the reflection's det(U Vs^T)", "reflection", det, 0.0);
    svd3_for_umeyama(rank1, U, Vs, sv, &det);
    check(sv[1] <= 0x1p-40 * sv[0], "svd3 the rank-1 case's sv_1", "rank1", sv[1], 0x1p-40 * sv[0]);
  }
  char name[32];
  for (int c = 0; c < 10; ++c) {
    double Sg[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Sg[i][j] = uniform();
    snprintf(name, sizeof name, "random %d", c);
    check_svd3(Sg, name);
  }

  double I4[4][4] = {}, rep4[4][4] = {}, r1[4][4];
  const double q[4] = {0.1, -0.5, 0.3, 0.8}, d4[4] = {2.0, 0.5, 2.0, -1.0};
  for (int i = 0; i < 4; ++i) {
    I4[i][i] = 1.0;
    rep4[i][i] = d4[i];
    for (int j = 0; j < 4; ++j) r1[i][j] = q[i] * q[j];
  }
  check_eig4(I4, "identity");
  check_eig4(rep4, "repeated");
  check_eig4(r1, "rank1");
  for (int c = 0; c < 10; ++c) {
    double A[4][4];
    for (int i = 0; i < 4; ++i)
      for (int j = i; j < 4; ++j) A[i][j] = A[j][i] = uniform();
    snprintf(name, sizeof name, "random %d", c);
    check_eig4(A, name);
  }
  if (failures) {
    printf("small_eig_host: %d checks failed\n", failures);
    return 1;
  }
  printf("small_eig_host: ok\n");
  return 0;
}
