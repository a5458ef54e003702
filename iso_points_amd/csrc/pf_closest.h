// The closest point of a triangle: the per-pair routine of pfdist.hip (the search and its backward pass) and of pfsign.hip
// (the sign of the distance), in one place so that both evaluate the same bits.  Host and device code, private to csrc/:
// iso_pfsign_pair runs it on the host for tests that pin the arithmetic without a GPU.
#pragma once
#include <math.h>

#pragma clang fp contract(off)

namespace {

// |p - (b0 v0 + b1 v1 + b2 v2)|^2
__host__ __device__ __forceinline__ float pf_d2_at(const float (&p)[3], const float (&v)[9], float b0, float b1, float b2) {
  const float rx = p[0] - ((b0 * v[0] + b1 * v[3]) + b2 * v[6]);
  const float ry = p[1] - ((b0 * v[1] + b1 * v[4]) + b2 * v[7]);
  const float rz = p[2] - ((b0 * v[2] + b1 * v[5]) + b2 * v[8]);
  return (rx * rx + ry * ry) + rz * rz;
}

// the parameter of the point of segment a + t (b - a), t in [0, 1], closest to p; a segment of no length gives 0
__host__ __device__ __forceinline__ float pf_edge_t(const float (&p)[3], const float* a, const float* b) {
  const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  const float dd = (dx * dx + dy * dy) + dz * dz;
  const float pd = ((p[0] - a[0]) * dx + (p[1] - a[1]) * dy) + (p[2] - a[2]) * dz;
  return dd > 0.f ? fminf(fmaxf(pd / dd, 0.f), 1.f) : 0.f;
}

// Squared distance from p to the closed triangle v = (v0, v1, v2) and the barycentric weights bw of the closest point.
// A triangle of area > min_area whose plane projection of p has no negative weight is measured at that projection;
// every other pair by the three edges (01, 12, 20; the first of equal distances).  A triangle without area never divides
// by its normal, so it gives no NaN.
__host__ __device__ __forceinline__ float pf_closest(const float (&p)[3], const float (&v)[9], float min_area, float (&bw)[3]) {
  const float e1x = v[3] - v[0], e1y = v[4] - v[1], e1z = v[5] - v[2];
  const float e2x = v[6] - v[0], e2y = v[7] - v[1], e2z = v[8] - v[2];
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float nn = (nx * nx + ny * ny) + nz * nz;
  if (0.5f * sqrtf(nn) > min_area) {
    const float wx = p[0] - v[0], wy = p[1] - v[1], wz = p[2] - v[2];
    // b1 = (w x e2) . n / n.n, b2 = (e1 x w) . n / n.n
    const float ax = wy * e2z - wz * e2y, ay = wz * e2x - wx * e2z, az = wx * e2y - wy * e2x;
    const float cx = e1y * wz - e1z * wy, cy = e1z * wx - e1x * wz, cz = e1x * wy - e1y * wx;
    const float b1 = ((ax * nx + ay * ny) + az * nz) / nn;
    const float b2 = ((cx * nx + cy * ny) + cz * nz) / nn;
    const float b0 = (1.0f - b1) - b2;
    if (b0 >= 0.f && b1 >= 0.f && b2 >= 0.f) {
      bw[0] = b0; bw[1] = b1; bw[2] = b2;
      return pf_d2_at(p, v, b0, b1, b2);
    }
  }
  const float t01 = pf_edge_t(p, &v[0], &v[3]);
  const float t12 = pf_edge_t(p, &v[3], &v[6]);
  const float t20 = pf_edge_t(p, &v[6], &v[0]);
  const float d01 = pf_d2_at(p, v, 1.0f - t01, t01, 0.f);
  const float d12 = pf_d2_at(p, v, 0.f, 1.0f - t12, t12);
  const float d20 = pf_d2_at(p, v, t20, 0.f, 1.0f - t20);
  float best = d01;
  bw[0] = 1.0f - t01; bw[1] = t01; bw[2] = 0.f;
  if (d12 < best) { best = d12; bw[0] = 0.f; bw[1] = 1.0f - t12; bw[2] = t12; }
  if (d20 < best) { best = d20; bw[0] = t20; bw[1] = 0.f; bw[2] = 1.0f - t20; }
  return best;
}

}  // namespace
