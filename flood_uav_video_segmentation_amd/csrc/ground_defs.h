// The rules of georeferencing the flood mosaic (ground_ops.hip; definitions: include/floodseg_test.h, ground_area, ground_rectify and
// ground_points).  Plain __host__ __device__ C++ with nothing of HIP in it, in the style of access_defs.h: the kernels call
// these functions, and a host program (tests/test_ground_cpu.py builds tests/ground_host_check.cpp) runs them on the CPU.  The same
// rules in numpy: tests/ground_ref.py.
//
// A MODEL is nine float64 (a0 a1 a2 b0 b1 b2 c0 c1 c2).  The FORWARD model takes anchor pixel coordinates (i, j) -- canvas lattice point
// (X, Y) is i = X - ox, j = Y - oy -- to millimetres east and north of a ground origin that only the host knows; the INVERSE model takes
// millimetres back to anchor coordinates.  Every floating-point statement below holds ONE operation, and the objects that include this
// header are built with -ffp-contract=off, so host and device round alike as long as the float64 division does (it is IEEE on both).
//
// WHY NOTHING LEAVES 63 BITS.  check_forward() holds before any launch.  (1) Every corner of the canvas lies within 2^31 mm of the
// origin, and a projective map with a positive denominator takes the canvas to the convex hull of its corners' images, so every
// lattice point does.  (2) One pixel's corner differences are below 2^30 (MAX_STEP), so each of the four shoelace products is below
// 2^60 and their sum below 2^62.  (3) Adjacent pixels share corners that were projected once, so the area2 of any set of pixels
// telescopes to the shoelace of the set's boundary.  The oriented area2 of all pixels of the canvas is therefore the shoelace of its
// border, which differs from the doubled area of the corners' quadrilateral, kept below 2^62 (MAX_AREA2), by at most the border's
// rounding: 2 * 16384 * 4 lattice points moved by a millimetre against edges shorter than 2^32, below 2^50.  A folded pixel's four
// corners lie within a few millimetres of each other (it folds by rounding only: the exact map keeps its orientation while the
// denominator is positive), so leaving out at most 2^28 of them changes a sum by less than 2^34.  Every partial sum of summed pixels --
// a class, a region, a workgroup's cell -- is a sum of positive terms of that total: below 2^62 + 2^50 + 2^34 < 2^63.
#ifndef FS_GROUND_DEFS_H_
#define FS_GROUND_DEFS_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FS_GND_HD __host__ __device__ __forceinline__
#else
#define FS_GND_HD inline
#endif

namespace fs {
namespace gnd {

constexpr int MAX_SIDE = 16384;                 // canvas and raster sides: 1..MAX_SIDE
constexpr int MAX_ORIGIN = 16384;               // |ox|, |oy|, as the mosaic ops
constexpr int MAX_GSD_MM = 1 << 20;             // gsd_mm: 1..2^20
constexpr int MAX_PLANES = 8;                   // uint8 planes of one ground_rectify call
constexpr int MAX_REGIONS = 65536;              // region_table's
constexpr double MAX_MM = 2147483648.0;         // |E|, |N| at the canvas corners stay below 2^31 mm
constexpr double MAX_STEP = 1073741824.0;       // one pixel's corner differences stay below 2^30 mm
constexpr double MAX_DENOM_RATIO = 4.0;         // largest / smallest corner denominator
constexpr double MAX_AREA2 = 4611686018427387904.0;  // 2^62: the doubled area of the canvas corners' quadrilateral stays below it
constexpr int64_t NO_POINT = INT64_MIN;         // ground_points: a point the model cannot place (denominator <= 0 or |mm| >= 2^53)
constexpr uint32_t UNSEEN = 255u;               // mosaic_resolve's class of a canvas pixel without votes

enum Refusal { OK = 0, NOT_FINITE = 1, DENOMINATOR = 2, RATIO = 3, RANGE = 4, STEP = 5, AREA = 6, ORIENTATION = 7 };

// ---- THE PROJECTION: three sums and two divisions, one operation per statement.  Both models use it.
FS_GND_HD double affine_sum(double k0, double k1, double k2, double i, double j) {
    const double p0 = k0 * i;
    const double p1 = k1 * j;
    const double s = p0 + p1;
    return s + k2;
}
FS_GND_HD double denominator(const double* m, double i, double j) { return affine_sum(m[6], m[7], m[8], i, j); }
FS_GND_HD void project(const double* m, double i, double j, double* u, double* v) {
    const double nu = affine_sum(m[0], m[1], m[2], i, j);
    const double nv = affine_sum(m[3], m[4], m[5], i, j);
    const double d = affine_sum(m[6], m[7], m[8], i, j);
    *u = nu / d;
    *v = nv / d;
}
FS_GND_HD double round_half_up(double q) {
    const double r = q + 0.5;
    return floor(r);
}

// ---- THE CORNER of lattice point (i, j) in anchor coordinates: millimetres as int64.  Every corner of every pixel, every vertex of
// ground_points and every check below goes through this function and nothing else.  The caller has run check_forward.
FS_GND_HD void corner(const double* fwd, int i, int j, int64_t* e, int64_t* n) {
    double qe, qn;
    project(fwd, (double)i, (double)j, &qe, &qn);
    *e = (int64_t)round_half_up(qe);
    *n = (int64_t)round_half_up(qn);
}
// the same for a point nobody has checked (ground_points): false where the model cannot place it
FS_GND_HD bool corner_checked(const double* fwd, int i, int j, int64_t* e, int64_t* n) {
    const double d = denominator(fwd, (double)i, (double)j);
    if (!(d > 0.0)) return false;
    double qe, qn;
    project(fwd, (double)i, (double)j, &qe, &qn);
    const double re = round_half_up(qe), rn = round_half_up(qn);
    if (!(fabs(re) < 9007199254740992.0) || !(fabs(rn) < 9007199254740992.0)) return false;
    *e = (int64_t)re, *n = (int64_t)rn;
    return true;
}

// ---- THE PIXEL'S AREA: the shoelace sum of its four corners in the order (i,j), (i+1,j), (i+1,j+1), (i,j+1), about the first: twice
// the signed area in mm^2, negative with north up.  Corner differences below 2^30: no product reaches 2^60.
FS_GND_HD int64_t area2(int64_t e0, int64_t n0, int64_t e1, int64_t n1, int64_t e2, int64_t n2, int64_t e3, int64_t n3) {
    const int64_t ux = e1 - e0, uy = n1 - n0, vx = e2 - e0, vy = n2 - n0, wx = e3 - e0, wy = n3 - n0;
    return (ux * vy - uy * vx) + (vx * wy - vy * wx);
}
// the model's orientation, taken at the anchor origin: the sign of the Jacobian's determinant there, det(M) / c2^3, c2 > 0.  -1 with north
// up and y down; 0 refuses the model.
FS_GND_HD int orientation(const double* m) {
    const double t0 = m[4] * m[8], t1 = m[5] * m[7], t2 = m[3] * m[8], t3 = m[5] * m[6], t4 = m[3] * m[7], t5 = m[4] * m[6];
    const double c0 = t0 - t1, c1 = t2 - t3, c2 = t4 - t5;
    const double d0 = m[0] * c0, d1 = m[1] * c1, d2 = m[2] * c2;
    const double s = d0 - d1;
    const double det = s + d2;
    return det > 0.0 ? 1 : det < 0.0 ? -1 : 0;
}
FS_GND_HD bool folded(int64_t oriented_area2) { return oriented_area2 <= 0; }

// ---- THE BOUNDS, enforced on the host before any launch.
FS_GND_HD bool finite9(const double* m) {
    for (int k = 0; k < 9; ++k)
        if (!(fabs(m[k]) <= 1.7976931348623157e308)) return false;  // false for NaN and the infinities
    return true;
}
// the denominator is affine, so its extremes over a box are at the box's corners: positive there means positive inside ("the horizon
// does not cross the map").  x0 <= x1, y0 <= y1 in the model's source coordinates.
FS_GND_HD int check_denominators(const double* m, double x0, double y0, double x1, double y1, double* dmin) {
    const double d[4] = {denominator(m, x0, y0), denominator(m, x1, y0), denominator(m, x1, y1), denominator(m, x0, y1)};
    double lo = d[0], hi = d[0];
    for (int k = 0; k < 4; ++k) {
        if (!(d[k] > 0.0)) return DENOMINATOR;
        lo = d[k] < lo ? d[k] : lo, hi = d[k] > hi ? d[k] : hi;
    }
    if (!(hi <= MAX_DENOM_RATIO * lo)) return RATIO;
    *dmin = lo;
    return OK;
}
// The forward model over the canvas whose lattice runs from (-ox, -oy) to (CW - ox, CH - oy).  The step bound: dE/di = (a0 - E c0) / d
// and dE/dj = (a1 - E c1) / d with |E| <= the largest |E| of the four corners and d >= dmin over the canvas, so one pixel's corner differences -- a step in i, one in j,
// or both -- stay below the sum of the two bounds, plus one for the rounding of the two ends.
FS_GND_HD int check_forward(const double* m, int CH, int CW, int ox, int oy) {
    if (!finite9(m)) return NOT_FINITE;
    if (orientation(m) == 0) return ORIENTATION;
    const double x0 = (double)(-ox), y0 = (double)(-oy), x1 = (double)(CW - ox), y1 = (double)(CH - oy);
    double dmin;
    const int r = check_denominators(m, x0, y0, x1, y1, &dmin);
    if (r != OK) return r;
    const double xs[4] = {x0, x1, x1, x0}, ys[4] = {y0, y0, y1, y1};
    double e[4], n[4];
    for (int k = 0; k < 4; ++k) {
        project(m, xs[k], ys[k], &e[k], &n[k]);
        if (!(fabs(e[k]) < MAX_MM - 1.0) || !(fabs(n[k]) < MAX_MM - 1.0)) return RANGE;
    }
    double emax = 0.0, nmax = 0.0;  // over the canvas too: it maps into the hull of its corners
    for (int k = 0; k < 4; ++k) emax = fabs(e[k]) > emax ? fabs(e[k]) : emax, nmax = fabs(n[k]) > nmax ? fabs(n[k]) : nmax;
    const double step_e = ((fabs(m[0]) + emax * fabs(m[6])) + (fabs(m[1]) + emax * fabs(m[7]))) / dmin;
    const double step_n = ((fabs(m[3]) + nmax * fabs(m[6])) + (fabs(m[4]) + nmax * fabs(m[7]))) / dmin;
    if (!(step_e + 1.0 < MAX_STEP) || !(step_n + 1.0 < MAX_STEP)) return STEP;
    double quad = 0.0;  // the doubled area of the corners' quadrilateral; each product is below 2^64, well inside a double's range
    for (int k = 0; k < 4; ++k) quad += e[k] * n[(k + 1) & 3] - e[(k + 1) & 3] * n[k];
    if (!(fabs(quad) < MAX_AREA2)) return AREA;
    return OK;
}
// The inverse model over the raster of GW x GH pixels of gsd_mm whose top-left ground corner is (e0_mm, ntop_mm).
FS_GND_HD int check_inverse(const double* m, int GH, int GW, int gsd_mm, int64_t e0_mm, int64_t ntop_mm) {
    if (!finite9(m)) return NOT_FINITE;
    const double x0 = (double)e0_mm, x1 = (double)(e0_mm + (int64_t)GW * gsd_mm), y1 = (double)ntop_mm, y0 = (double)(ntop_mm - (int64_t)GH * gsd_mm);
    double dmin;
    return check_denominators(m, x0, y0, x1, y1, &dmin);
}

// ---- RECTIFICATION.  The ground point under the centre of raster pixel (u, v): every value is a multiple of half a millimetre below
// 2^53, so the three statements are exact.
FS_GND_HD void raster_ground(int u, int v, int gsd_mm, int64_t e0_mm, int64_t ntop_mm, double* eg, double* ng) {
    const double cu = (double)u + 0.5, cv = (double)v + 0.5;
    const double du = cu * (double)gsd_mm, dv = cv * (double)gsd_mm;
    *eg = (double)e0_mm + du;
    *ng = (double)ntop_mm - dv;
}
// the anchor coordinates under a ground point; false where they are not numbers a canvas could hold
FS_GND_HD bool ground_to_anchor(const double* inv, double eg, double ng, double* x, double* y) {
    project(inv, eg, ng, x, y);
    return fabs(*x) < 1048576.0 && fabs(*y) < 1048576.0;  // false for NaN too; canvas coordinates are below 2^15 + 2^14
}
// nearest sampling: the canvas pixel that holds anchor point (x, y); false outside the canvas.  The caller has ground_to_anchor's yes.
FS_GND_HD bool nearest_pixel(double x, double y, int ox, int oy, int CH, int CW, int* X, int* Y) {
    *X = (int)floor(x) + ox, *Y = (int)floor(y) + oy;
    return *X >= 0 && *X < CW && *Y >= 0 && *Y < CH;
}
// colour: the four taps start at floor(x - 0.5), the weights are Q8 from floor(frac * 256)
FS_GND_HD void colour_taps(double x, double y, int ox, int oy, int* X0, int* Y0, uint32_t* wx, uint32_t* wy) {
    const double sx = x - 0.5, sy = y - 0.5;
    const double fx = floor(sx), fy = floor(sy);
    const double rx = sx - fx, ry = sy - fy;
    const double qx = rx * 256.0, qy = ry * 256.0;
    *X0 = (int)fx + ox, *Y0 = (int)fy + oy;
    *wx = (uint32_t)floor(qx), *wy = (uint32_t)floor(qy);  // 0..255
}
FS_GND_HD bool seen(uint32_t rgba) { return (rgba >> 24) != 0u; }
// the integer blend of one channel (shift 0, 8 or 16) of the four taps: the weights sum to 65536
FS_GND_HD uint32_t blend_channel(uint32_t t00, uint32_t t10, uint32_t t01, uint32_t t11, uint32_t wx, uint32_t wy, int shift) {
    const uint32_t ax = 256u - wx, ay = 256u - wy;
    const uint32_t sum = ax * ay * ((t00 >> shift) & 0xFFu) + wx * ay * ((t10 >> shift) & 0xFFu) + ax * wy * ((t01 >> shift) & 0xFFu) +
                         wx * wy * ((t11 >> shift) & 0xFFu);  // <= 65536 * 255
    return (sum + 32768u) >> 16;
}
// One raster pixel's colour (r | g << 8 | b << 16).  `tap(X, Y)` answers with the canvas' rgba word, 0 (unseen) off the canvas.  A tap
// that is unseen or off the canvas makes the pixel fall back to the nearest tap; an unseen nearest tap gives the fill.
template <class Tap>
FS_GND_HD uint32_t rectify_colour(const Tap& tap, double x, double y, int ox, int oy, uint32_t rgb_fill) {
    int X0, Y0;
    uint32_t wx, wy;
    colour_taps(x, y, ox, oy, &X0, &Y0, &wx, &wy);
    const uint32_t t00 = tap(X0, Y0), t10 = tap(X0 + 1, Y0), t01 = tap(X0, Y0 + 1), t11 = tap(X0 + 1, Y0 + 1);
    if (seen(t00) && seen(t10) && seen(t01) && seen(t11))
        return blend_channel(t00, t10, t01, t11, wx, wy, 0) | (blend_channel(t00, t10, t01, t11, wx, wy, 8) << 8) |
               (blend_channel(t00, t10, t01, t11, wx, wy, 16) << 16);
    const uint32_t near = tap((int)floor(x) + ox, (int)floor(y) + oy);
    return seen(near) ? (near & 0xFFFFFFu) : (rgb_fill & 0xFFFFFFu);
}
// A raster tile is EMPTY when the anchor points under its four lattice corners all lie beyond the same side of the canvas box grown by
// one pixel: the inverse model with a positive denominator takes the tile into the convex hull of those four points, so every sample
// of the tile lies beyond that side too, where the nearest pixel and every tap are off the canvas.  x, y: the four points; the box is
// the canvas in anchor coordinates.
FS_GND_HD bool tile_outside(const double* x, const double* y, int ox, int oy, int CH, int CW) {
    const double left = (double)(-ox) - 1.0, right = (double)(CW - ox) + 1.0, top = (double)(-oy) - 1.0, bottom = (double)(CH - oy) + 1.0;
    bool l = true, r = true, t = true, b = true;
    for (int k = 0; k < 4; ++k) {
        l = l && x[k] < left, r = r && x[k] > right, t = t && y[k] < top, b = b && y[k] > bottom;  // false for NaN: such a tile is not skipped
    }
    return l || r || t || b;
}

}  // namespace gnd
}  // namespace fs
#endif  // FS_GROUND_DEFS_H_
