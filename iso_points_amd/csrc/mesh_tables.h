// Marching tetrahedra on the Kuhn split, in numbers: the slots, the six tetrahedra, the 16 triangle cases derived at compile
// time, the inside test and the vertex on a slot (include/isopoints.h section N).  One copy for the dense kernels
// (mesh_extract.hip) and the block-sparse ones (mesh_extract_sparse.hip, section O): the two meshes are the same bits
// because the rule is the same text.
#pragma once
#include <float.h>
#include "iso_common.h"

#pragma clang fp contract(off)

namespace {

// ---- the Kuhn split, in numbers ----------------------------------------------------------------------------------------
// An offset inside a cell is a 3-bit code (x = 1, y = 2, z = 4).  Slots in their order +x +y +z +xy +xz +yz +xyz; a cell's
// corner c is the cell's own point (c = 0) or the far end of its slot c - 1, so a point's active mask is its cell's
// corner mask shifted down by one.
constexpr int kSlotCode[7] = {1, 2, 4, 3, 5, 6, 7};
constexpr int slot_of_code(int code) { return code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 3 ? 3 : code == 5 ? 4 : code == 6 ? 5 : 6; }
constexpr int corner_of_code(int code) { return code == 0 ? 0 : slot_of_code(code) + 1; }

// Tetrahedron T of a cell: 000 -> +e_a -> +e_a+e_b -> 111 for the T-th permutation (a, b, c) of the axes in lexicographic
// order.  det[P1-P0, P2-P0, P3-P0] = det[e_a, e_b, e_c] = the sign of the permutation: T = 1, 2, 5 are the odd ones.
constexpr int kPerm[6][2] = {{0, 1}, {0, 2}, {1, 0}, {1, 2}, {2, 0}, {2, 1}};       // (a, b); c is the third
constexpr bool tet_odd(int T) { return T == 1 || T == 2 || T == 5; }
constexpr int tet_code(int T, int u) {                                             // offset code of corner u of T
  return u == 0 ? 0 : u == 1 ? (1 << kPerm[T][0]) : u == 2 ? ((1 << kPerm[T][0]) | (1 << kPerm[T][1])) : 7;
}
// A tetrahedron's edges (u, v), u < v, in the order 01 02 03 12 13 23.  All six run from a lower to a higher grid point, so
// edge (u, v) is slot (code_v - code_u) of the point at corner u.
constexpr int kEdgeU[6] = {0, 0, 0, 1, 1, 2}, kEdgeV[6] = {1, 2, 3, 2, 3, 3};
constexpr int edge_id(int x, int y) {
  const int u = x < y ? x : y, v = x < y ? y : x;
  return u == 0 ? v - 1 : u == 1 ? v + 1 : 5;
}
constexpr uint32_t tet_owner_pack(int T) {                 // 3 bits per edge: offset code of the owning corner
  uint32_t r = 0;
  for (int e = 0; e < 6; ++e) r |= (uint32_t)tet_code(T, kEdgeU[e]) << (3 * e);
  return r;
}
constexpr uint32_t tet_slot_pack(int T) {                  // 3 bits per edge: the slot at the owner
  uint32_t r = 0;
  for (int e = 0; e < 6; ++e) r |= (uint32_t)slot_of_code(tet_code(T, kEdgeV[e]) ^ tet_code(T, kEdgeU[e])) << (3 * e);
  return r;
}

constexpr int perm_sign4(int a, int b, int c, int d) {
  const int p[4] = {a, b, c, d};
  int s = 1;
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (p[i] > p[j]) s = -s;
  return s;
}

// The triangles of a tetrahedron with inside mask m (bit u = corner u inside): the count in bits 0-1, then 3 bits per
// triangle corner, each the id of the tetrahedron edge that carries the vertex.
//   One corner A apart from B < C < D: the normal of (AB, AC, AD) is t2 t3 det[B-A, C-A, D-A] along B - A (and likewise along
//   C - A, D - A), so it points away from A iff that determinant is positive.  Away is outwards if A is the inside corner.
//   A < B inside, C < D outside: the quad AC, AD, BD, BC is cut along AC-BD; the normal of (AC, AD, BD) dotted with C - A is
//   u (1 - w) det[B-A, C-A, D-A], outwards iff positive; the second half (AC, BD, BC) is the same fan.
//   det[B-A, C-A, D-A] = the tetrahedron's orientation times the sign of the permutation (A, B, C, D) of its corners.
// A negative product swaps the last two corners of every triangle.
constexpr uint32_t tri_code(int m, bool odd) {
  int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
  for (int q = 0; q < 4; ++q) {
    if ((m >> q) & 1) in[ni++] = q; else out[no++] = q;
  }
  if (ni == 0 || ni == 4) return 0u;
  const int orient = odd ? -1 : 1;
  int e[6] = {0, 0, 0, 0, 0, 0}, n = 1;
  bool flip = false;
  if (ni == 2) {
    const int A = in[0], B = in[1], C = out[0], D = out[1];
    n = 2;
    e[0] = edge_id(A, C); e[1] = edge_id(A, D); e[2] = edge_id(B, D);
    e[3] = edge_id(A, C); e[4] = edge_id(B, D); e[5] = edge_id(B, C);
    flip = orient * perm_sign4(A, B, C, D) < 0;
  } else {
    const bool lone_in = ni == 1;
    const int A = lone_in ? in[0] : out[0];
    const int* r = lone_in ? out : in;
    e[0] = edge_id(A, r[0]); e[1] = edge_id(A, r[1]); e[2] = edge_id(A, r[2]);
    const bool away = orient * perm_sign4(A, r[0], r[1], r[2]) > 0;
    flip = away != lone_in;
  }
  if (flip) {
    int t = e[1]; e[1] = e[2]; e[2] = t;
    t = e[4]; e[4] = e[5]; e[5] = t;
  }
  uint32_t code = (uint32_t)n;
  for (int c = 0; c < 3 * n; ++c) code |= (uint32_t)e[c] << (2 + 3 * c);
  return code;
}
struct TriTable { uint32_t v[2][16]; };
constexpr TriTable make_tri_table() {
  TriTable t = {};
  for (int m = 0; m < 16; ++m) { t.v[0][m] = tri_code(m, false); t.v[1][m] = tri_code(m, true); }
  return t;
}
__constant__ TriTable kTri = make_tri_table();

// ---- device helpers ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mt_finite(float x) { return fabsf(x) <= FLT_MAX; }          // false for NaN and +-inf
__device__ __forceinline__ unsigned mt_inside(float v, float iso) { return (v < iso && mt_finite(v)) ? 1u : 0u; }

// the inside mask of tetrahedron T from the cell's corner mask
template <int T>
__device__ __forceinline__ unsigned tet_mask(unsigned cm) {
  constexpr int c1 = corner_of_code(tet_code(T, 1)), c2 = corner_of_code(tet_code(T, 2));
  return (cm & 1u) | (((cm >> c1) & 1u) << 1) | (((cm >> c2) & 1u) << 2) | (((cm >> 7) & 1u) << 3);
}
__device__ __forceinline__ int tet_tris(unsigned m) {
  const int pc = __popc(m);
  return pc == 2 ? 2 : (pc & 1);
}
__device__ __forceinline__ int cell_tris(unsigned cm) {
  return tet_tris(tet_mask<0>(cm)) + tet_tris(tet_mask<1>(cm)) + tet_tris(tet_mask<2>(cm)) + tet_tris(tet_mask<3>(cm)) +
         tet_tris(tet_mask<4>(cm)) + tet_tris(tet_mask<5>(cm));
}

// which corners of the cell at a point exist (bit c), from whether the point has a successor along x, y, z
__device__ __forceinline__ unsigned exist_mask(bool ex, bool ey, bool ez) {
  return 1u | (ex ? 0x02u : 0u) | (ey ? 0x04u : 0u) | (ez ? 0x08u : 0u) | (ex && ey ? 0x10u : 0u) | (ex && ez ? 0x20u : 0u) |
         (ey && ez ? 0x40u : 0u) | (ex && ey && ez ? 0x80u : 0u);
}

struct MtGrid {
  int nx, ny, nz;
  float org[3], spc[3], iso;
};

// position of grid point idx along axis d: one multiplication, one addition
__device__ __forceinline__ float mt_pos(const MtGrid& g, int d, int idx) { return g.org[d] + (float)idx * g.spc[d]; }

// the vertex of the slot with offset `code` at grid point (i, j, k): va at the owning end, vb at the far one
__device__ __forceinline__ void mt_vertex(const MtGrid& g, int i, int j, int k, int code, float va, float vb, float (&out)[3]) {
  const float t = (mt_finite(va) && mt_finite(vb)) ? (g.iso - va) / (vb - va) : 0.5f;
  const float pa[3] = {mt_pos(g, 0, i), mt_pos(g, 1, j), mt_pos(g, 2, k)};
  const float pb[3] = {mt_pos(g, 0, i + (code & 1)), mt_pos(g, 1, j + ((code >> 1) & 1)), mt_pos(g, 2, k + (code >> 2))};
#pragma unroll
  for (int d = 0; d < 3; ++d) out[d] = pa[d] + t * (pb[d] - pa[d]);
}

}  // namespace
