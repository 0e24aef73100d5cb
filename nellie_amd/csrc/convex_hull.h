// Host only, no HIP: the exact convex hull behind the solidity columns.  Included by
// nellie_hip_branchfeat.hip and by tools/convex_hull_check.cpp, which runs it under the host sanitizers.
//
// skimage's convex_hull_image(offset_coordinates=True) takes the hull of every voxel centre moved by +-1/2 along one axis.  In
// doubled coordinates everything is an integer: a voxel c (relative to its region's box) gives the 2 D points 2 c +- e_a, lattice
// point x of the box is 2 x.  The hull of the moved points is hull(centres) + diamond, so only the vertices of the centres' own hull
// are moved: ch_facets() takes that hull first (it fails exactly when the centres have affine rank < 3, skimage's all-zero convex
// image), then the hull of the moved vertices.  A 2-D region is the prism over its polygon (the moved points at Z = -1 and Z = +1),
// cut at Z = 0, so one builder serves both; a prism is never flat, as a 2-D region is never degenerate.
//
// Arithmetic: box-relative coordinates are < 2^15 (the engine refuses wider frames), doubled and moved ones lie in [-1, 2^16), their
// differences are below 2^17 in magnitude, a normal (a cross product of two differences) has components below 2^35, and N . p and
// N . (p - q) stay below 3 * 2^35 * 2^17 < 2^54: int64 suffices everywhere, nothing is rounded.
//
// The builder is the incremental one: a starting tetrahedron, then every point that lies strictly outside some triangle removes the
// triangles it sees and closes the hole from the horizon.  A point in the plane of a triangle does not see it, so coplanar points
// cost nothing and leave coplanar triangles, which ch_facets() merges by their reduced plane (N / gcd, d / gcd).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <array>
#include <vector>

namespace nl_convex {

typedef long long ci64;                                 // 64 bits, the engine's i64
struct Pt { ci64 z, y, x; };
struct Facet { ci64 nz, ny, nx, d; };                 // inside: nz Z + ny Y + nx X <= d, in doubled box-relative coordinates
static inline bool operator<(const Facet &a, const Facet &b) {
    return std::array<ci64, 4>{a.nz, a.ny, a.nx, a.d} < std::array<ci64, 4>{b.nz, b.ny, b.nx, b.d};
}
static inline bool operator==(const Facet &a, const Facet &b) { return a.nz == b.nz && a.ny == b.ny && a.nx == b.nx && a.d == b.d; }

static inline Pt ch_sub(const Pt &a, const Pt &b) { return Pt{a.z - b.z, a.y - b.y, a.x - b.x}; }
static inline Pt ch_cross(const Pt &a, const Pt &b) { return Pt{a.y * b.x - a.x * b.y, a.x * b.z - a.z * b.x, a.z * b.y - a.y * b.z}; }
static inline ci64 ch_dot(const Pt &a, const Pt &b) { return a.z * b.z + a.y * b.y + a.x * b.x; }
static inline bool ch_zero(const Pt &a) { return a.z == 0 && a.y == 0 && a.x == 0; }

struct Tri { int a, b, c; Pt n; ci64 d; };            // outward normal n, n . p == d on the triangle

static inline Tri ch_tri(const std::vector<Pt> &p, int a, int b, int c) {
    Tri t{a, b, c, ch_cross(ch_sub(p[b], p[a]), ch_sub(p[c], p[a])), 0};
    t.d = ch_dot(t.n, p[a]);
    return t;
}

// The triangles of the hull of p; false when the points have affine rank < 3 (no hull).
static inline bool ch_hull(const std::vector<Pt> &p, std::vector<Tri> &tris) {
    tris.clear();
    const int n = (int)p.size();
    int i1 = -1, i2 = -1, i3 = -1;
    for (int i = 1; i < n && i1 < 0; ++i)
        if (!ch_zero(ch_sub(p[i], p[0]))) i1 = i;
    if (i1 < 0) return false;
    const Pt e1 = ch_sub(p[i1], p[0]);
    Pt nrm{0, 0, 0};
    for (int i = 1; i < n && i2 < 0; ++i) {
        nrm = ch_cross(e1, ch_sub(p[i], p[0]));
        if (!ch_zero(nrm)) i2 = i;
    }
    if (i2 < 0) return false;
    ci64 side = 0;
    for (int i = 1; i < n && i3 < 0; ++i) {
        side = ch_dot(nrm, ch_sub(p[i], p[0]));
        if (side != 0) i3 = i;
    }
    if (i3 < 0) return false;
    int a = 0, b = i1, c = i2;
    if (side > 0) std::swap(b, c);                    // the fourth point lies below (a, b, c)
    tris.push_back(ch_tri(p, a, b, c));
    tris.push_back(ch_tri(p, b, a, i3));
    tris.push_back(ch_tri(p, c, b, i3));
    tris.push_back(ch_tri(p, a, c, i3));
    std::vector<uint64_t> edges;
    std::vector<int> order((size_t)n);                // candidates arrive sorted by (z, y, x), the order in which every point lies
    for (int i = 0; i < n; ++i) order[(size_t)i] = i; // outside the hull so far: a fixed shuffle (the same for the same input) puts most
    uint64_t rnd = 0x9e3779b97f4a7c15ull;             // points inside early.  The facet planes do not depend on the order.
    for (int i = n - 1; i > 0; --i) {
        rnd ^= rnd << 13; rnd ^= rnd >> 7; rnd ^= rnd << 17;
        std::swap(order[(size_t)i], order[(size_t)(rnd % (uint64_t)(i + 1))]);
    }
    for (int q : order) {
        if (q == 0 || q == i1 || q == i2 || q == i3) continue;
        edges.clear();
        size_t keep = 0;
        for (size_t k = 0; k < tris.size(); ++k) {
            const Tri t = tris[k];
            if (ch_dot(t.n, p[q]) > t.d) {
                edges.push_back(((uint64_t)(uint32_t)t.a << 32) | (uint32_t)t.b);
                edges.push_back(((uint64_t)(uint32_t)t.b << 32) | (uint32_t)t.c);
                edges.push_back(((uint64_t)(uint32_t)t.c << 32) | (uint32_t)t.a);
            } else {
                tris[keep++] = t;
            }
        }
        if (edges.empty()) continue;
        tris.resize(keep);
        std::sort(edges.begin(), edges.end());
        for (uint64_t e : edges)                      // an edge of the hole whose other side was not seen: the horizon
            if (!std::binary_search(edges.begin(), edges.end(), (e << 32) | (e >> 32)))
                tris.push_back(ch_tri(p, (int)(e >> 32), (int)(e & 0xffffffffu), q));
    }
    return true;
}

static inline ci64 ch_gcd(ci64 a, ci64 b) {
    a = a < 0 ? -a : a;
    b = b < 0 ? -b : b;
    while (b) { const ci64 t = a % b; a = b; b = t; }
    return a;
}

// The facets of one region from its candidate voxel centres c (box-relative, (n, ndim) rows: (z, y, x) or (y, x)), appended to
// `out`; none when a 3-D region has affine rank < 3.  Any superset of the hull's vertices among the region's voxels will do.
static inline void ch_facets(const ci64 *c, ci64 n, int ndim, std::vector<Facet> &out) {
    std::vector<Pt> pts, moved;
    std::vector<Tri> tris;
    if (ndim == 3) {
        pts.reserve((size_t)n);
        for (ci64 i = 0; i < n; ++i) pts.push_back(Pt{2 * c[3 * i], 2 * c[3 * i + 1], 2 * c[3 * i + 2]});
        if (!ch_hull(pts, tris)) return;
        std::vector<char> used(pts.size(), 0);
        for (const Tri &t : tris) used[t.a] = used[t.b] = used[t.c] = 1;
        for (size_t i = 0; i < pts.size(); ++i) {
            if (!used[i]) continue;
            const Pt q = pts[i];
            for (int s = -1; s <= 1; s += 2) {
                moved.push_back(Pt{q.z + s, q.y, q.x});
                moved.push_back(Pt{q.z, q.y + s, q.x});
                moved.push_back(Pt{q.z, q.y, q.x + s});
            }
        }
    } else {
        for (ci64 i = 0; i < n; ++i)
            for (int Z = -1; Z <= 1; Z += 2)
                for (int s = -1; s <= 1; s += 2) {
                    moved.push_back(Pt{Z, 2 * c[2 * i] + s, 2 * c[2 * i + 1]});
                    moved.push_back(Pt{Z, 2 * c[2 * i], 2 * c[2 * i + 1] + s});
                }
    }
    if (!ch_hull(moved, tris)) return;                // cannot fail: the moved points of one voxel already span space
    std::vector<Facet> f;
    f.reserve(tris.size());
    for (const Tri &t : tris) {
        if (ndim == 2 && t.n.y == 0 && t.n.x == 0) continue;           // the prism's two lids hold at Z = 0
        const ci64 g = ch_gcd(ch_gcd(t.n.z, t.n.y), t.n.x);
        f.push_back(Facet{t.n.z / g, t.n.y / g, t.n.x / g, t.d / g}); // d = N . v is a multiple of g as N is
    }
    std::sort(f.begin(), f.end());
    f.erase(std::unique(f.begin(), f.end()), f.end());
    out.insert(out.end(), f.begin(), f.end());
}

}  // namespace nl_convex
