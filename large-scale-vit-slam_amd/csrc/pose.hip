// Per-chunk pose / Sim(3) composition of FeatureAlignedVGGT.forward
// (featureAligned_vggt.py:96-143, 187-196) as one launch: the (B, S, 4, 4)
// SE(3) chain, the Markley quaternion mean over the overlap (geometry.py:4-37,
// a 4x4 symmetric eigenproblem solved by cyclic Jacobi on the device) and the
// final pose encoding -- no host round trip per chunk.
//
// One 64-lane workgroup per batch element; lane f (stride 64) owns frame f.
// All pose algebra in fp32 as the reference (autocast is disabled there,
// featureAligned_vggt.py:104), except the FoV round trip (tan, atan: fp64,
// rounded once); the Jacobi sweeps run in fp64 and the unit
// eigenvector is rounded to fp32 like torch.linalg.eigh's fp32 result (its
// sign is arbitrary in both, SURVEY Appendix A.7 -- and irrelevant here: the
// mean only enters through quat_to_mat, which is even in q).
#include "common.h"
#include "small_eig.h"

namespace {

struct Aff {  // rows 0..2 of a 4x4 SE(3) / Sim(3) matrix, row 3 = (0, 0, 0, 1)
  float r[3][3];
  float t[3];
};

// VGGT rotation.quat_to_mat: scalar-last (x, y, z, w), 2 / |q|^2 scaling
__device__ void quat_to_mat(const float* q, float R[3][3]) {
  const float i = q[0], j = q[1], k = q[2], r = q[3];
  const float two_s = 2.0f / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  R[0][0] = 1.f - two_s * (j * j + k * k);
  R[0][1] = two_s * (i * j - k * r);
  R[0][2] = two_s * (i * k + j * r);
  R[1][0] = two_s * (i * j + k * r);
  R[1][1] = 1.f - two_s * (i * i + k * k);
  R[1][2] = two_s * (j * k - i * r);
  R[2][0] = two_s * (i * k - j * r);
  R[2][1] = two_s * (j * k + i * r);
  R[2][2] = 1.f - two_s * (i * i + j * j);
}

__device__ __forceinline__ float sqrt_pos(float x) { return x > 0.f ? sqrtf(x) : 0.f; }

// VGGT rotation.mat_to_quat: the best-conditioned of the four candidates,
// divided by 2 max(|q_i|, 0.1), reordered to (x, y, z, w), w >= 0
__device__ void mat_to_quat(const float R[3][3], float* q) {
  const float m00 = R[0][0], m01 = R[0][1], m02 = R[0][2], m10 = R[1][0], m11 = R[1][1], m12 = R[1][2],
              m20 = R[2][0], m21 = R[2][1], m22 = R[2][2];
  float qa[4] = {sqrt_pos(1.f + m00 + m11 + m22), sqrt_pos(1.f + m00 - m11 - m22), sqrt_pos(1.f - m00 + m11 - m22),
                 sqrt_pos(1.f - m00 - m11 + m22)};
  int b = 0;
  for (int i = 1; i < 4; ++i)
    if (qa[i] > qa[b]) b = i;  // first maximum, as torch.argmax
  float c[4];  // (w, x, y, z)
  switch (b) {
    case 0: c[0] = qa[0] * qa[0]; c[1] = m21 - m12; c[2] = m02 - m20; c[3] = m10 - m01; break;
    case 1: c[0] = m21 - m12; c[1] = qa[1] * qa[1]; c[2] = m10 + m01; c[3] = m02 + m20; break;
    case 2: c[0] = m02 - m20; c[1] = m10 + m01; c[2] = qa[2] * qa[2]; c[3] = m12 + m21; break;
    default: c[0] = m10 - m01; c[1] = m20 + m02; c[2] = m21 + m12; c[3] = qa[3] * qa[3]; break;
  }
  const float d = 2.0f * fmaxf(qa[b], 0.1f);
  float x = c[1] / d, y = c[2] / d, z = c[3] / d, w = c[0] / d;
  if (w < 0.f) { x = -x; y = -y; z = -z; w = -w; }
  q[0] = x; q[1] = y; q[2] = z; q[3] = w;
}

__device__ __forceinline__ void normalize4(float* q) {
  const float n = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-8f);
  for (int i = 0; i < 4; ++i) q[i] = q[i] / n;
}

// aligned_vggt/utils/data.py:33-52: [T, quat] -> SE(3), quat normalised first
__device__ Aff enc_to_aff(const float* e) {
  float q[4] = {e[3], e[4], e[5], e[6]};
  normalize4(q);
  Aff a;
  quat_to_mat(q, a.r);
  a.t[0] = e[0]; a.t[1] = e[1]; a.t[2] = e[2];
  return a;
}

__device__ Aff mul(const Aff& a, const Aff& b) {  // a @ b
  Aff o;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o.r[i][j] = a.r[i][0] * b.r[0][j] + a.r[i][1] * b.r[1][j] + a.r[i][2] * b.r[2][j];
    o.t[i] = a.r[i][0] * b.t[0] + a.r[i][1] * b.t[1] + a.r[i][2] * b.t[2] + a.t[i];
  }
  return o;
}

// VGGT geometry.closed_form_inverse_se3: [R^T | -R^T t]
__device__ Aff inv_se3(const Aff& a) {
  Aff o;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o.r[i][j] = a.r[j][i];
  for (int i = 0; i < 3; ++i) o.t[i] = -(o.r[i][0] * a.t[0] + o.r[i][1] * a.t[1] + o.r[i][2] * a.t[2]);
  return o;
}

constexpr int MAX_OV = 64;

__global__ __launch_bounds__(64) void pose_compose_kernel(
    const float* __restrict__ chunk_sim3, const float* __restrict__ frame_se3, const float* __restrict__ cam,
    const float* __restrict__ ctx, int S_prev, const float* __restrict__ gt_first, int S, int ov, float H, float W,
    float* __restrict__ out, float* __restrict__ pt_out) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  __shared__ Aff s_chunk, s_ident, s_mean, s_ptid;
  __shared__ float s_scale;
  __shared__ float s_ct[MAX_OV][7];  // overlap transforms as [t, quat] (Markley input)
  const float* cs = chunk_sim3 + (int64_t)b * 8;
  const float* cb = cam + (int64_t)b * S * 9;
  if (lane == 0) {
    s_chunk = enc_to_aff(cs);  // featureAligned_vggt.py:97
    s_scale = cs[7];           // :98
    // pose_encoding_to_extri_intri (VGGT): quat_to_mat on the raw quaternion
    Aff e0;
    quat_to_mat(cb + 3, e0.r);
    e0.t[0] = cb[0]; e0.t[1] = cb[1]; e0.t[2] = cb[2];
    s_ptid = e0;               // point_identity_alignment, :115
    s_ident = inv_se3(e0);     // :114
  }
  __syncthreads();
  // camera extrinsics of frame f: re-centred on frame 0, translation scaled (:109-119)
  auto extr = [&](int f) {
    const float* c = cb + (int64_t)f * 9;
    Aff e;
    quat_to_mat(c + 3, e.r);
    e.t[0] = c[0]; e.t[1] = c[1]; e.t[2] = c[2];
    e = mul(e, s_ident);
    for (int i = 0; i < 3; ++i) e.t[i] *= s_scale;
    return e;
  };
  // initial chunk alignment (:121-137)
  if (ctx == nullptr) {
    if (lane == 0) {
      Aff I;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) I.r[i][j] = i == j ? 1.f : 0.f;
        I.t[i] = 0.f;
      }
      s_mean = I;
    }
  } else if (gt_first != nullptr) {
    if (lane == 0) {
      const float* g = gt_first + (int64_t)b * 16;
      Aff m;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m.r[i][j] = g[i * 4 + j];
        m.t[i] = g[i * 4 + 3];
      }
      s_mean = m;
    }
  } else {
    const float* cx = ctx + (int64_t)b * S_prev * 9;
    for (int k = lane; k < ov; k += 64) {
      const Aff co = enc_to_aff(cx + (int64_t)(S_prev - ov + k) * 9);  // context pose_enc[-1][:, -ov:], :126
      const Aff ct = mul(inv_se3(extr(k)), co);                      // :127-128
      if (ov == 1) {
        s_mean = ct;                                                   // :135
      } else {                                                         // extri_to_pose_encoding (data.py:12-30)
        float q[4];
        mat_to_quat(ct.r, q);
        normalize4(q);
        s_ct[k][0] = ct.t[0]; s_ct[k][1] = ct.t[1]; s_ct[k][2] = ct.t[2];
        for (int i = 0; i < 4; ++i) s_ct[k][3 + i] = q[i];
      }
    }
    __syncthreads();
    if (ov > 1 && lane == 0) {  // averagePoseEncodings (geometry.py:4-37)
      float t[3] = {0.f, 0.f, 0.f};
      for (int k = 0; k < ov; ++k)
        for (int i = 0; i < 3; ++i) t[i] += s_ct[k][i];
      const float inv_n = 1.0f / (float)ov;
      float M[4][4] = {};
      for (int k = 0; k < ov; ++k) {
        float q[4] = {s_ct[k][3], s_ct[k][4], s_ct[k][5], s_ct[k][6]};
        normalize4(q);
        for (int i = 0; i < 4; ++i)
          for (int j = 0; j < 4; ++j) M[i][j] += inv_n * (q[i] * q[j]);
      }
      double Md[4][4], v[4];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) Md[i][j] = M[i][j];
      top_eigvec4(Md, v);
      float e[7] = {t[0] / (float)ov, t[1] / (float)ov, t[2] / (float)ov, (float)v[0], (float)v[1], (float)v[2],
                    (float)v[3]};
      s_mean = enc_to_aff(e);  // pose_encoding_to_extri(mean), :133
    }
  }
  __syncthreads();
  // per-frame SE(3) (:99-101), composed with the mean transform (:139) and the
  // camera extrinsics (:142), then encoded with the camera FoV (:143)
  const float* fb = frame_se3 + (int64_t)b * (S - 1) * 7;
  for (int f = lane; f < S; f += 64) {
    Aff pf = f == 0 ? s_chunk : mul(enc_to_aff(fb + (int64_t)(f - 1) * 7), s_chunk);
    pf = mul(pf, s_mean);
    const Aff a = mul(extr(f), pf);
    float q[4];
    mat_to_quat(a.r, q);
    const float* c = cb + (int64_t)f * 9;
    // pose_encoding_to_extri_intri -> intrinsics -> extri_intri_to_pose_encoding
    // (in fp64, rounded once: tanf / atanf and two divisions are up to 4.5 x further from the
    // exact value than the same fp32 steps with a correctly rounded libm)
    const double fy = ((double)H / 2.0) / tan((double)c[7] / 2.0);
    const double fx = ((double)W / 2.0) / tan((double)c[8] / 2.0);
    float* o = out + ((int64_t)b * S + f) * 9;
    o[0] = a.t[0]; o[1] = a.t[1]; o[2] = a.t[2];
    o[3] = q[0]; o[4] = q[1]; o[5] = q[2]; o[6] = q[3];
    o[7] = (float)(2.0 * atan(((double)H / 2.0) / fy));
    o[8] = (float)(2.0 * atan(((double)W / 2.0) / fx));
    if (f == 0 && pt_out != nullptr) {
      // point transform (:188-195): context ? inv(per_frame_se3[:, 0]) @ ptid : ptid
      const Aff p = ctx != nullptr ? mul(inv_se3(pf), s_ptid) : s_ptid;
      float* po = pt_out + (int64_t)b * 16;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) po[i * 4 + j] = p.r[i][j];
        po[i * 4 + 3] = p.t[i];
      }
      po[12] = 0.f; po[13] = 0.f; po[14] = 0.f; po[15] = 1.f;
    }
  }
}

// Per-chunk pose algebra of the pose-aligned VGGT (poseAligned_wrapped_vggt.py:74-130,
// 172-177) as one launch: re-centring on the first frame, the GT scale of the
// translations (:84-104, scale_lse_solver), the mean transform (identity | GT first
// pose | Markley mean over the overlap), the aligned encoding and the point transform.
// Same layout as pose_compose_kernel: one 64-lane workgroup per batch element, lane-stride
// over frames.  The GT scale |sum x.y / sum x^2| is taken in fp64 from the raw encodings
// (per-lane partials, combined by lane 0 in lane order: no atomics, independent of the
// grid), the quotient rounded to fp32 once; everything else is fp32 as the reference's, the
// translations take one fp32 multiply.
__global__ __launch_bounds__(64) void pose_align_kernel(
    const float* __restrict__ cam, const float* __restrict__ ctx, int S_prev, const float* __restrict__ gt, int S,
    int ov, float H, float W, float* __restrict__ out, float* __restrict__ pt_out, float* __restrict__ scales) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  __shared__ Aff s_ident, s_mean, s_ptid;
  __shared__ float s_scale;
  __shared__ double s_part[64][2];
  __shared__ float s_ct[MAX_OV][7];  // overlap transforms as [t, quat] (Markley input)
  const float* cb = cam + (int64_t)b * S * 9;
  const float* gb = gt != nullptr ? gt + (int64_t)b * S * 12 : nullptr;
  auto gt_aff = [&](int f) {  // gt_poses[b, f] (3 x 4, row-major)
    const float* g = gb + (int64_t)f * 12;
    Aff m;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) m.r[i][j] = g[i * 4 + j];
      m.t[i] = g[i * 4 + 3];
    }
    return m;
  };
  if (lane == 0) {
    // pose_encoding_to_extri_intri (VGGT): quat_to_mat on the raw quaternion
    Aff e0;
    quat_to_mat(cb + 3, e0.r);
    e0.t[0] = cb[0]; e0.t[1] = cb[1]; e0.t[2] = cb[2];
    s_ptid = e0;               // point_identity_alignment, :80
    s_ident = inv_se3(e0);     // :79
  }
  __syncthreads();
  // camera extrinsics of frame f re-centred on frame 0 (:81), translation not yet scaled.  Frame 0
  // takes lane 0's matrix: a second evaluation of quat_to_mat may be contracted differently, and
  // R0 R0^T is symmetric (an exact identity quaternion, as the reference's) only for one R0.
  auto extr = [&](int f) {
    if (f == 0) return mul(s_ptid, s_ident);
    const float* c = cb + (int64_t)f * 9;
    Aff e;
    quat_to_mat(c + 3, e.r);
    e.t[0] = c[0]; e.t[1] = c[1]; e.t[2] = c[2];
    return mul(e, s_ident);
  };
  if (gb != nullptr) {  // :92-104
    // The operands of the scale in fp64 from the raw encodings: the re-centring cancels
    // (x_f = R_f (-R0^T t0) + t_f), and taken in fp32 its rounding, not that of the sums, decides
    // how far the scale is from the exact one (up to 2 x the fp32 restatement's error).
    auto rot64 = [](const float* q, double R[3][3]) {  // quat_to_mat in fp64
      const double i = q[0], j = q[1], k = q[2], r = q[3];
      const double two_s = 2.0 / (i * i + j * j + k * k + r * r);
      R[0][0] = 1.0 - two_s * (j * j + k * k); R[0][1] = two_s * (i * j - k * r); R[0][2] = two_s * (i * k + j * r);
      R[1][0] = two_s * (i * j + k * r); R[1][1] = 1.0 - two_s * (i * i + k * k); R[1][2] = two_s * (j * k - i * r);
      R[2][0] = two_s * (i * k - j * r); R[2][1] = two_s * (j * k + i * r); R[2][2] = 1.0 - two_s * (i * i + j * j);
    };
    double R0[3][3], tinv[3], ginv[3];  // the translations of inv(extr[0]) and inv(gt[0])
    rot64(cb + 3, R0);
    for (int i = 0; i < 3; ++i) {
      tinv[i] = -(R0[0][i] * (double)cb[0] + R0[1][i] * (double)cb[1] + R0[2][i] * (double)cb[2]);
      ginv[i] = -((double)gb[i] * (double)gb[3] + (double)gb[4 + i] * (double)gb[7] + (double)gb[8 + i] * (double)gb[11]);
    }
    double sxy = 0.0, sxx = 0.0;
    for (int f = lane; f < S; f += 64) {
      const float* c = cb + (int64_t)f * 9;
      const float* g = gb + (int64_t)f * 12;
      double R[3][3];
      rot64(c + 3, R);
      for (int i = 0; i < 3; ++i) {
        const double x = R[i][0] * tinv[0] + R[i][1] * tinv[1] + R[i][2] * tinv[2] + (double)c[i];
        const double y = (double)g[i * 4] * ginv[0] + (double)g[i * 4 + 1] * ginv[1] + (double)g[i * 4 + 2] * ginv[2]
                         + (double)g[i * 4 + 3];
        sxy += x * y;
        sxx += x * x;
      }
    }
    s_part[lane][0] = sxy;
    s_part[lane][1] = sxx;
    __syncthreads();
    if (lane == 0) {
      double a = 0.0, d = 0.0;
      for (int k = 0; k < 64; ++k) {
        a += s_part[k][0];
        d += s_part[k][1];
      }
      s_scale = fabsf((float)(a / d));  // 0 / 0: NaN, kept
    }
  } else if (lane == 0) {
    s_scale = 1.0f;
  }
  // mean transform (:107-126)
  if (ctx == nullptr) {
    if (lane == 0) {
      Aff I;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) I.r[i][j] = i == j ? 1.f : 0.f;
        I.t[i] = 0.f;
      }
      s_mean = I;
    }
  } else if (gb != nullptr) {
    if (lane == 0) s_mean = gt_aff(0);  // gt_poses[:, :1], not centred (:109)
  } else {
    const float* cx = ctx + (int64_t)b * S_prev * 9;
    for (int k = lane; k < ov; k += 64) {
      const Aff co = enc_to_aff(cx + (int64_t)(S_prev - ov + k) * 9);  // context pose_enc[-1][:, -ov:], :111
      const Aff ct = mul(inv_se3(extr(k)), co);                      // :113-115
      if (ov == 1) {
        s_mean = ct;                                                   // :124
      } else {                                                         // extri_to_pose_encoding (data.py:12-30)
        float q[4];
        mat_to_quat(ct.r, q);
        normalize4(q);
        s_ct[k][0] = ct.t[0]; s_ct[k][1] = ct.t[1]; s_ct[k][2] = ct.t[2];
        for (int i = 0; i < 4; ++i) s_ct[k][3 + i] = q[i];
      }
    }
    __syncthreads();
    if (ov > 1 && lane == 0) {  // averagePoseEncodings (geometry.py:4-37)
      float t[3] = {0.f, 0.f, 0.f};
      for (int k = 0; k < ov; ++k)
        for (int i = 0; i < 3; ++i) t[i] += s_ct[k][i];
      const float inv_n = 1.0f / (float)ov;
      float M[4][4] = {};
      for (int k = 0; k < ov; ++k) {
        float q[4] = {s_ct[k][3], s_ct[k][4], s_ct[k][5], s_ct[k][6]};
        normalize4(q);
        for (int i = 0; i < 4; ++i)
          for (int j = 0; j < 4; ++j) M[i][j] += inv_n * (q[i] * q[j]);
      }
      double Md[4][4], v[4];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) Md[i][j] = M[i][j];
      top_eigvec4(Md, v);
      float e[7] = {t[0] / (float)ov, t[1] / (float)ov, t[2] / (float)ov, (float)v[0], (float)v[1], (float)v[2],
                    (float)v[3]};
      s_mean = enc_to_aff(e);  // pose_encoding_to_extri(mean), :122
    }
  }
  __syncthreads();
  const float scale = s_scale;
  if (lane == 0) {
    scales[b] = scale;
    if (pt_out != nullptr) {
      // point transform (:171-177): context ? inv(mean) @ ptid : ptid
      const Aff p = ctx != nullptr ? mul(inv_se3(s_mean), s_ptid) : s_ptid;
      float* po = pt_out + (int64_t)b * 16;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) po[i * 4 + j] = p.r[i][j];
        po[i * 4 + 3] = p.t[i];
      }
      po[12] = 0.f; po[13] = 0.f; po[14] = 0.f; po[15] = 1.f;
    }
  }
  // scaled extrinsics composed with the mean transform (:129), encoded with the camera FoV (:130)
  for (int f = lane; f < S; f += 64) {
    Aff e = extr(f);
    for (int i = 0; i < 3; ++i) e.t[i] *= scale;  // :102
    Aff a = mul(e, s_mean);
    // the reference's 4 x 4 product adds extr[i][3] * mean[3][j] = t_i * 0 to the rotation: +0 for a
    // finite translation, NaN under a NaN scale (0 / 0) -- the quaternion is NaN there too
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) a.r[i][j] += e.t[i] * 0.f;
    float q[4];
    mat_to_quat(a.r, q);
    const float* c = cb + (int64_t)f * 9;
    // the FoV round trip in fp64, rounded once (as pose_compose_kernel)
    const double fy = ((double)H / 2.0) / tan((double)c[7] / 2.0);
    const double fx = ((double)W / 2.0) / tan((double)c[8] / 2.0);
    float* o = out + ((int64_t)b * S + f) * 9;
    o[0] = a.t[0]; o[1] = a.t[1]; o[2] = a.t[2];
    o[3] = q[0]; o[4] = q[1]; o[5] = q[2]; o[6] = q[3];
    o[7] = (float)(2.0 * atan(((double)H / 2.0) / fy));
    o[8] = (float)(2.0 * atan(((double)W / 2.0) / fx));
  }
}

// ---- GT alignment of a merged sequence from its poses (alignment.py:131-242, :325-370, :6-59)

// One 64-lane workgroup per batch element, lane-stride over frames.  Sums are per-lane fp64
// partials combined by lane 0 in lane order (no atomics, independent of the grid), every result is
// rounded to fp32 once.  enc / enc_out are not __restrict__: enc_out may be enc (every read of the
// first W frames' centres is behind a barrier, and a lane reads frame f's row before it writes it).
__global__ __launch_bounds__(64) void gt_pose_align_kernel(const float* enc, int ew, const float* __restrict__ gt,
                                                           int S, int W, int mode, float H, float Wimg,
                                                           float* __restrict__ scales, float* __restrict__ transform,
                                                           float* enc_out) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const float* eb = enc + (int64_t)b * S * ew;
  const float* gb = gt + (int64_t)b * S * 12;
  __shared__ double s_part[64][10];
  __shared__ double s_mean[6];
  __shared__ Aff s_T;
  __shared__ float s_c;
  if (mode == VGGT_GT_POSE_PER_FRAME) {  // alignment.py:131-165
    for (int f = lane; f < S; f += 64) {
      const float* e = eb + (int64_t)f * ew;
      const float* g = gb + (int64_t)f * 12;
      double sxy = 0.0, sxx = 0.0;
      for (int i = 0; i < 3; ++i) {
        sxy += (double)e[i] * (double)g[i * 4 + 3];
        sxx += (double)e[i] * (double)e[i];
      }
      scales[(int64_t)b * S + f] = f == 0 ? 1.0f : fabsf((float)(sxy / sxx));  // 0 / 0: NaN, kept
    }
    return;
  }
  if (mode == VGGT_GT_POSE_SCALE) {  // alignment.py:206-242 (scale_lse_solver over the first W frames)
    double sxy = 0.0, sxx = 0.0;
    for (int f = lane; f < W; f += 64) {
      const float* e = eb + (int64_t)f * ew;
      const float* g = gb + (int64_t)f * 12;
      for (int i = 0; i < 3; ++i) {
        sxy += (double)e[i] * (double)g[i * 4 + 3];
        sxx += (double)e[i] * (double)e[i];
      }
    }
    s_part[lane][0] = sxy;
    s_part[lane][1] = sxx;
    __syncthreads();
    if (lane == 0) {
      double a = 0.0, d = 0.0;
      for (int k = 0; k < 64; ++k) {
        a += s_part[k][0];
        d += s_part[k][1];
      }
      scales[b] = fabsf((float)(a / d));  // 0 / 0: NaN, kept
    }
    return;
  }
  // SIM3 (alignment.py:325-370): Umeyama over the first W camera centres -R^T t, in fp64 from the
  // fp32 inputs (the prediction's rotation from the raw quaternion, as pose_encoding_to_extri_intri)
  auto centres = [&](int f, double* x, double* y) {
    const float* e = eb + (int64_t)f * ew;
    const float* g = gb + (int64_t)f * 12;
    const double qi = e[3], qj = e[4], qk = e[5], qr = e[6];
    const double two_s = 2.0 / (qi * qi + qj * qj + qk * qk + qr * qr);
    double R[3][3];
    R[0][0] = 1.0 - two_s * (qj * qj + qk * qk); R[0][1] = two_s * (qi * qj - qk * qr); R[0][2] = two_s * (qi * qk + qj * qr);
    R[1][0] = two_s * (qi * qj + qk * qr); R[1][1] = 1.0 - two_s * (qi * qi + qk * qk); R[1][2] = two_s * (qj * qk - qi * qr);
    R[2][0] = two_s * (qi * qk - qj * qr); R[2][1] = two_s * (qj * qk + qi * qr); R[2][2] = 1.0 - two_s * (qi * qi + qj * qj);
    for (int i = 0; i < 3; ++i) {
      x[i] = -(R[0][i] * (double)e[0] + R[1][i] * (double)e[1] + R[2][i] * (double)e[2]);
      y[i] = -((double)g[i] * (double)g[3] + (double)g[4 + i] * (double)g[7] + (double)g[8 + i] * (double)g[11]);
    }
  };
  double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int f = lane; f < W; f += 64) {
    double x[3], y[3];
    centres(f, x, y);
    for (int i = 0; i < 3; ++i) {
      acc[i] += x[i];
      acc[3 + i] += y[i];
    }
  }
  for (int j = 0; j < 6; ++j) s_part[lane][j] = acc[j];
  __syncthreads();
  if (lane == 0) {
    for (int j = 0; j < 6; ++j) {
      double a = 0.0;
      for (int k = 0; k < 64; ++k) a += s_part[k][j];
      s_mean[j] = a / (double)W;
    }
  }
  __syncthreads();
  for (int j = 0; j < 10; ++j) acc[j] = 0.0;
  for (int f = lane; f < W; f += 64) {
    double x[3], y[3];
    centres(f, x, y);
    for (int i = 0; i < 3; ++i) {
      x[i] -= s_mean[i];
      y[i] -= s_mean[3 + i];
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) acc[3 * i + j] += y[i] * x[j];
    acc[9] += x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  }
  for (int j = 0; j < 10; ++j) s_part[lane][j] = acc[j];
  __syncthreads();
  if (lane == 0) {
    double s2[10];
    for (int j = 0; j < 10; ++j) {
      double a = 0.0;
      for (int k = 0; k < 64; ++k) a += s_part[k][j];
      s2[j] = a / (double)W;
    }
    double Sg[3][3], R[3][3], c;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Sg[i][j] = s2[3 * i + j];
    umeyama3(Sg, s2[9], R, &c);
    Aff T;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) T.r[i][j] = (float)R[i][j];
      T.t[i] = (float)(s_mean[3 + i] - c * (R[i][0] * s_mean[0] + R[i][1] * s_mean[1] + R[i][2] * s_mean[2]));
    }
    s_T = T;
    s_c = (float)c;
    float* to = transform + (int64_t)b * 16;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) to[i * 4 + j] = T.r[i][j];
      to[i * 4 + 3] = T.t[i];
    }
    to[12] = 0.f; to[13] = 0.f; to[14] = 0.f; to[15] = 1.f;
    scales[b] = (float)c;
  }
  if (enc_out == nullptr) return;
  __syncthreads();
  // apply_sim3_alignment (alignment.py:449-489, :528-594) on every frame, fp32 as the reference:
  // w2c -> c2w, translation x scale, T ., -> w2c, mat_to_quat; the FoV round trip as pose_compose_kernel
  const Aff T = s_T;
  const float c = s_c;
  for (int f = lane; f < S; f += 64) {
    const float* e = eb + (int64_t)f * ew;
    float in[9];
    for (int i = 0; i < 9; ++i) in[i] = e[i];
    Aff w;
    quat_to_mat(in + 3, w.r);
    w.t[0] = in[0]; w.t[1] = in[1]; w.t[2] = in[2];
    Aff p = inv_se3(w);
    for (int i = 0; i < 3; ++i) p.t[i] *= c;
    const Aff a = inv_se3(mul(T, p));
    float q[4];
    mat_to_quat(a.r, q);
    const double fy = ((double)H / 2.0) / tan((double)in[7] / 2.0);
    const double fx = ((double)Wimg / 2.0) / tan((double)in[8] / 2.0);
    float* o = enc_out + ((int64_t)b * S + f) * 9;
    o[0] = a.t[0]; o[1] = a.t[1]; o[2] = a.t[2];
    o[3] = q[0]; o[4] = q[1]; o[5] = q[2]; o[6] = q[3];
    o[7] = (float)(2.0 * atan(((double)H / 2.0) / fy));
    o[8] = (float)(2.0 * atan(((double)Wimg / 2.0) / fx));
  }
}

// ---- ATE / RPE / scale-consistency terms of one update (trajectory_metrics.py:28-48, :154-182, :306-331)

struct M4 {
  double m[4][4];
};

__device__ M4 load4(const float* p) {
  M4 a;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) a.m[i][j] = (double)p[i * 4 + j];
  return a;
}

__device__ M4 mul4(const M4& a, const M4& b) {
  M4 o;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      o.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j] + a.m[i][3] * b.m[3][j];
  return o;
}

// General 4x4 inverse by the adjugate over 2x2 sub-determinants (no pivot search, so no
// run-time indexing); det == 0 gives inf / NaN entries.
__device__ M4 inv4(const M4& A) {
  const double(*a)[4] = A.m;
  const double s0 = a[0][0] * a[1][1] - a[1][0] * a[0][1], s1 = a[0][0] * a[1][2] - a[1][0] * a[0][2];
  const double s2 = a[0][0] * a[1][3] - a[1][0] * a[0][3], s3 = a[0][1] * a[1][2] - a[1][1] * a[0][2];
  const double s4 = a[0][1] * a[1][3] - a[1][1] * a[0][3], s5 = a[0][2] * a[1][3] - a[1][2] * a[0][3];
  const double c5 = a[2][2] * a[3][3] - a[3][2] * a[2][3], c4 = a[2][1] * a[3][3] - a[3][1] * a[2][3];
  const double c3 = a[2][1] * a[3][2] - a[3][1] * a[2][2], c2 = a[2][0] * a[3][3] - a[3][0] * a[2][3];
  const double c1 = a[2][0] * a[3][2] - a[3][0] * a[2][2], c0 = a[2][0] * a[3][1] - a[3][0] * a[2][1];
  const double inv = 1.0 / (s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0);
  M4 o;
  o.m[0][0] = (a[1][1] * c5 - a[1][2] * c4 + a[1][3] * c3) * inv;
  o.m[0][1] = (-a[0][1] * c5 + a[0][2] * c4 - a[0][3] * c3) * inv;
  o.m[0][2] = (a[3][1] * s5 - a[3][2] * s4 + a[3][3] * s3) * inv;
  o.m[0][3] = (-a[2][1] * s5 + a[2][2] * s4 - a[2][3] * s3) * inv;
  o.m[1][0] = (-a[1][0] * c5 + a[1][2] * c2 - a[1][3] * c1) * inv;
  o.m[1][1] = (a[0][0] * c5 - a[0][2] * c2 + a[0][3] * c1) * inv;
  o.m[1][2] = (-a[3][0] * s5 + a[3][2] * s2 - a[3][3] * s1) * inv;
  o.m[1][3] = (a[2][0] * s5 - a[2][2] * s2 + a[2][3] * s1) * inv;
  o.m[2][0] = (a[1][0] * c4 - a[1][1] * c2 + a[1][3] * c0) * inv;
  o.m[2][1] = (-a[0][0] * c4 + a[0][1] * c2 - a[0][3] * c0) * inv;
  o.m[2][2] = (a[3][0] * s4 - a[3][1] * s2 + a[3][3] * s0) * inv;
  o.m[2][3] = (-a[2][0] * s4 + a[2][1] * s2 - a[2][3] * s0) * inv;
  o.m[3][0] = (-a[1][0] * c3 + a[1][1] * c1 - a[1][2] * c0) * inv;
  o.m[3][1] = (a[0][0] * c3 - a[0][1] * c1 + a[0][2] * c0) * inv;
  o.m[3][2] = (-a[3][0] * s3 + a[3][1] * s1 - a[3][2] * s0) * inv;
  o.m[3][3] = (a[2][0] * s3 - a[2][1] * s1 + a[2][2] * s0) * inv;
  return o;
}

// One 64-lane workgroup per sequence, lane-stride over frames (ATE, scale factor) and over the
// pairs (i, i + delta) (RPE).  No sums: every output element is an fp64 function of at most four
// input poses, rounded to fp32 once.
__global__ __launch_bounds__(64) void trajectory_errors_kernel(
    const float* __restrict__ pred, const float* __restrict__ gt, int S, int delta, float* __restrict__ ate_vec,
    float* __restrict__ ate_norm, float* __restrict__ rpe_trans, float* __restrict__ rpe_rot,
    float* __restrict__ scale_factor) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const float* pb = pred + (int64_t)b * S * 16;
  const float* gb = gt + (int64_t)b * S * 16;
  if (ate_vec != nullptr || ate_norm != nullptr || scale_factor != nullptr) {
    for (int f = lane; f < S; f += 64) {
      const float* p = pb + (int64_t)f * 16;
      const float* g = gb + (int64_t)f * 16;
      const double px = p[3], py = p[7], pz = p[11], gx = g[3], gy = g[7], gz = g[11];
      const double dx = px - gx, dy = py - gy, dz = pz - gz;
      if (ate_vec != nullptr) {
        float* o = ate_vec + ((int64_t)b * S + f) * 3;
        o[0] = (float)dx; o[1] = (float)dy; o[2] = (float)dz;
      }
      if (ate_norm != nullptr) ate_norm[(int64_t)b * S + f] = (float)sqrt(dx * dx + dy * dy + dz * dz);
      if (scale_factor != nullptr && f > 0)  // clamp_min(1e-8) on an fp32 tensor: the fp32 value of 1e-8
        scale_factor[(int64_t)b * (S - 1) + f - 1] =
            (float)((gx * px + gy * py + gz * pz) / fmax(px * px + py * py + pz * pz, (double)1e-8f));
    }
  }
  if ((rpe_trans == nullptr && rpe_rot == nullptr) || S <= delta) return;
  const int n = S - delta;
  for (int i = lane; i < n; i += 64) {
    const M4 pr = mul4(inv4(load4(pb + (int64_t)i * 16)), load4(pb + (int64_t)(i + delta) * 16));
    const M4 gr = mul4(inv4(load4(gb + (int64_t)i * 16)), load4(gb + (int64_t)(i + delta) * 16));
    const M4 err = mul4(inv4(gr), pr);
    if (rpe_trans != nullptr)
      rpe_trans[(int64_t)b * n + i] =
          (float)sqrt(err.m[0][3] * err.m[0][3] + err.m[1][3] * err.m[1][3] + err.m[2][3] * err.m[2][3]);
    if (rpe_rot != nullptr) {
      const double c = (err.m[0][0] + err.m[1][1] + err.m[2][2] - 1.0) / 2.0;
      // torch.clamp keeps a NaN (fmin / fmax would drop it): both comparisons are false for one
      rpe_rot[(int64_t)b * n + i] = (float)acos(c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c));
    }
  }
}

}  // namespace

extern "C" int vggt_gt_pose_align(const float* pose_enc, int enc_width, const float* gt_extr, int B, int S, int W,
                                  int mode, int img_h, int img_w, float* scales, float* transform,
                                  float* pose_enc_out, void* stream) {
  if (B <= 0 || S <= 0 || !pose_enc || !gt_extr || !scales) return VGGT_ERR_SHAPE;
  if (enc_width != 7 && enc_width != 9) return VGGT_ERR_SHAPE;
  if (mode != VGGT_GT_POSE_SCALE && mode != VGGT_GT_POSE_PER_FRAME && mode != VGGT_GT_POSE_SIM3)
    return VGGT_ERR_UNSUPPORTED;
  if (W == -1) W = S;
  if (W < 1 || W > S) return VGGT_ERR_SHAPE;
  if (mode == VGGT_GT_POSE_SIM3) {
    if (enc_width != 9) return VGGT_ERR_UNSUPPORTED;  // the reference decodes a 9-wide encoding here
    if (!transform || (pose_enc_out != nullptr && (img_h <= 0 || img_w <= 0))) return VGGT_ERR_SHAPE;
  }
  gt_pose_align_kernel<<<B, 64, 0, (hipStream_t)stream>>>(pose_enc, enc_width, gt_extr, S, W, mode, (float)img_h,
                                                          (float)img_w, scales, transform,
                                                          mode == VGGT_GT_POSE_SIM3 ? pose_enc_out : nullptr);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

extern "C" int vggt_trajectory_errors(const float* pred_c2w, const float* gt_c2w, int B, int S, int delta,
                                      float* ate_vec, float* ate_norm, float* rpe_trans, float* rpe_rot,
                                      float* scale_factor, void* stream) {
  if (B <= 0 || S <= 0 || delta < 1 || !pred_c2w || !gt_c2w) return VGGT_ERR_SHAPE;
  trajectory_errors_kernel<<<B, 64, 0, (hipStream_t)stream>>>(pred_c2w, gt_c2w, S, delta, ate_vec, ate_norm,
                                                              rpe_trans, rpe_rot, scale_factor);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

extern "C" int vggt_pose_align(const float* cam_pose_enc, const float* ctx_pose_enc, int S_prev, const float* gt,
                               int B, int S, int overlap, int H, int W, float* aligned_pose_enc,
                               float* point_transform, float* scales, void* stream) {
  if (B <= 0 || S <= 0 || H <= 0 || W <= 0) return VGGT_ERR_SHAPE;
  if (!cam_pose_enc || !aligned_pose_enc || !scales) return VGGT_ERR_SHAPE;
  if (gt != nullptr && S == 1) return VGGT_ERR_SHAPE;  // the reference defines no scale for one frame
  if (ctx_pose_enc != nullptr && gt == nullptr) {
    if (overlap < 1 || overlap > S || overlap > S_prev || overlap > MAX_OV) return VGGT_ERR_SHAPE;
  }
  pose_align_kernel<<<B, 64, 0, (hipStream_t)stream>>>(cam_pose_enc, ctx_pose_enc, S_prev, gt, S, overlap, (float)H,
                                                       (float)W, aligned_pose_enc, point_transform, scales);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

extern "C" int vggt_pose_compose(const float* chunk_sim3, const float* frame_se3, const float* cam_pose_enc,
                                 const float* ctx_pose_enc, int S_prev, const float* gt_first, int B, int S,
                                 int overlap, int H, int W, float* aligned_pose_enc, float* point_transform,
                                 void* stream) {
  if (B <= 0 || S <= 0 || H <= 0 || W <= 0) return VGGT_ERR_SHAPE;
  if (!chunk_sim3 || !cam_pose_enc || !aligned_pose_enc || (S > 1 && !frame_se3)) return VGGT_ERR_SHAPE;
  if (ctx_pose_enc != nullptr && gt_first == nullptr) {
    if (overlap < 1 || overlap > S || overlap > S_prev || overlap > MAX_OV) return VGGT_ERR_SHAPE;
  }
  pose_compose_kernel<<<B, 64, 0, (hipStream_t)stream>>>(chunk_sim3, frame_se3, cam_pose_enc, ctx_pose_enc, S_prev,
                                                         gt_first, S, overlap, (float)H, (float)W, aligned_pose_enc,
                                                         point_transform);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}
