// pnp_dev.h — the per-lane arithmetic of the absolute-pose RANSAC (pnp_ransac.hip): the skip predicates, the P3P
// and the known-rotation minimal solvers and the inlier test, all f64 with + - * / and sqrt only (the unit is built
// with -ffp-contract=off).  Nothing here indexes a local array by a run-time value: selections are written as
// conditional moves, so that the hypothesis kernel keeps its state in registers.
#pragma once
#include <hip/hip_runtime.h>

namespace vio360 {

#define PNP_HD __host__ __device__ __forceinline__

constexpr double kPnpCollinear2 = 1e-10;  // sin^2 of the angle at the first point below which three points are collinear
constexpr int kPnpCubicSteps = 40;        // Newton steps on the pencil's cubic
constexpr int kPnpPolishSteps = 5;        // Gauss-Newton steps on the three distance constraints

struct PnpV3 {
    double x, y, z;
};
PNP_HD PnpV3 pv(double x, double y, double z) { return PnpV3{x, y, z}; }
PNP_HD PnpV3 padd(PnpV3 a, PnpV3 b) { return pv(a.x + b.x, a.y + b.y, a.z + b.z); }
PNP_HD PnpV3 psub(PnpV3 a, PnpV3 b) { return pv(a.x - b.x, a.y - b.y, a.z - b.z); }
PNP_HD PnpV3 pscale(double s, PnpV3 a) { return pv(s * a.x, s * a.y, s * a.z); }
PNP_HD double pdot(PnpV3 a, PnpV3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
PNP_HD PnpV3 pcross(PnpV3 a, PnpV3 b) {
    return pv(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
PNP_HD bool pfinite(double v) { return v - v == 0.0; }
PNP_HD bool pfinite3(PnpV3 a) { return pfinite(a.x) && pfinite(a.y) && pfinite(a.z); }
PNP_HD double pabs(double v) { return v < 0.0 ? -v : v; }
PNP_HD double pdet(PnpV3 a, PnpV3 b, PnpV3 c) { return pdot(a, pcross(b, c)); }

// symmetric 3x3
struct PnpS3 {
    double a00, a01, a02, a11, a12, a22;
};
PNP_HD PnpV3 scol0(PnpS3 m) { return pv(m.a00, m.a01, m.a02); }
PNP_HD PnpV3 scol1(PnpS3 m) { return pv(m.a01, m.a11, m.a12); }
PNP_HD PnpV3 scol2(PnpS3 m) { return pv(m.a02, m.a12, m.a22); }
PNP_HD PnpV3 smul(PnpS3 m, PnpV3 v) { return pv(pdot(scol0(m), v), pdot(scol1(m), v), pdot(scol2(m), v)); }
PNP_HD PnpS3 saxpy(PnpS3 a, double g, PnpS3 b) {
    return PnpS3{a.a00 + g * b.a00, a.a01 + g * b.a01, a.a02 + g * b.a02,
                 a.a11 + g * b.a11, a.a12 + g * b.a12, a.a22 + g * b.a22};
}

// x = R p + t, each row ((R0*p0 + R1*p1) + R2*p2) + t
PNP_HD PnpV3 pnp_transform(const double* R, const double* t, PnpV3 p) {
    return pv(((R[0] * p.x + R[1] * p.y) + R[2] * p.z) + t[0], ((R[3] * p.x + R[4] * p.y) + R[5] * p.z) + t[1],
              ((R[6] * p.x + R[7] * p.y) + R[8] * p.z) + t[2]);
}

// the inlier test of both modes: the angle between b and x is at most the threshold (c2 = cos^2 of it).  A NaN
// anywhere makes the point a non-inlier.
PNP_HD bool pnp_inlier(PnpV3 x, PnpV3 b, double c2) {
    const double d = pdot(b, x);
    return d > 0.0 && d * d >= c2 * pdot(x, x);
}

// two sampled bearings closer than the minimum pair angle (cp2 = cos^2 of it); the same form as the inlier test
PNP_HD bool pnp_pair_close(PnpV3 bi, PnpV3 bj, double cp2) {
    const double d = pdot(bi, bj);
    return d > 0.0 && d * d >= cp2 * (pdot(bi, bi) * pdot(bj, bj));
}

// coincident or collinear world points: with e1 = p2 - p1, e2 = p3 - p1 and c = e1 x e2, the row is kept only
// when c.c > kPnpCollinear2 * ((e1.e1) * (e2.e2)) (false for a zero e1 or e2 and for NaN)
PNP_HD bool pnp_collinear(PnpV3 p1, PnpV3 p2, PnpV3 p3) {
    const PnpV3 e1 = psub(p2, p1), e2 = psub(p3, p1), c = pcross(e1, e2);
    return !(pdot(c, c) > kPnpCollinear2 * (pdot(e1, e1) * pdot(e2, e2)));
}

// one real root of x^3 + b x^2 + c x + d: Newton from outside the stationary points (monotone from there), or
// from the inflection point of a monotone cubic
PNP_HD double pnp_cubic_root(double b, double c, double d) {
    double r;
    const double disc = b * b - 3.0 * c;
    if (disc >= 0.0) {
        const double v = sqrt(disc);
        const double t1 = (-b - v) / 3.0;
        double k = ((t1 + b) * t1 + c) * t1 + d;
        if (k > 0.0) {
            const double q = -k / (3.0 * t1 + b);
            r = t1 - sqrt(q > 0.0 ? q : 0.0);
        } else {
            const double t2 = (-b + v) / 3.0;
            k = ((t2 + b) * t2 + c) * t2 + d;
            const double q = -k / (3.0 * t2 + b);
            r = t2 + sqrt(q > 0.0 ? q : 0.0);
        }
    } else {
        r = -b / 3.0;
    }
    for (int it = 0; it < kPnpCubicSteps; ++it) {
        const double f = ((r + b) * r + c) * r + d;
        const double fp = (3.0 * r + 2.0 * b) * r + c;
        if (f == 0.0 || fp == 0.0) break;
        r = r - f / fp;
    }
    return r;
}

struct PnpTri {  // one sample's geometry
    double a12, a13, a23, b12, b13, b23;
};

// Gauss-Newton on the three distance constraints; false when the depths end up non-finite or not positive
PNP_HD bool pnp_polish(const PnpTri& g, double& l1, double& l2, double& l3) {
    for (int it = 0; it < kPnpPolishSteps; ++it) {
        const double r1 = ((l1 * l1 + l2 * l2) - 2.0 * g.b12 * (l1 * l2)) - g.a12;
        const double r2 = ((l1 * l1 + l3 * l3) - 2.0 * g.b13 * (l1 * l3)) - g.a13;
        const double r3 = ((l2 * l2 + l3 * l3) - 2.0 * g.b23 * (l2 * l3)) - g.a23;
        // J = [j11 j12 0; j21 0 j23; 0 j32 j33]
        const double j11 = 2.0 * (l1 - g.b12 * l2), j12 = 2.0 * (l2 - g.b12 * l1);
        const double j21 = 2.0 * (l1 - g.b13 * l3), j23 = 2.0 * (l3 - g.b13 * l1);
        const double j32 = 2.0 * (l2 - g.b23 * l3), j33 = 2.0 * (l3 - g.b23 * l2);
        const double det = -(j11 * (j23 * j32)) - j12 * (j21 * j33);
        if (!(pabs(det) > 0.0) || !pfinite(det)) break;
        // delta = J^-1 r by the adjugate
        const double d1 = (-(j23 * j32) * r1 - (j12 * j33) * r2 + (j12 * j23) * r3) / det;
        const double d2 = (-(j21 * j33) * r1 + (j11 * j33) * r2 - (j11 * j23) * r3) / det;
        const double d3 = ((j21 * j32) * r1 - (j11 * j32) * r2 - (j12 * j21) * r3) / det;
        l1 -= d1;
        l2 -= d2;
        l3 -= d3;
    }
    return pfinite(l1) && pfinite(l2) && pfinite(l3) && l1 > 0.0 && l2 > 0.0 && l3 > 0.0;
}

// R = Y X^-1 with X = [p1-p2, p2-p3, cross], Y the same of the scaled bearings; t = l1 y1 - R p1
PNP_HD bool pnp_pose_from_depths(PnpV3 p1, PnpV3 p2, PnpV3 p3, PnpV3 y1, PnpV3 y2, PnpV3 y3, double l1, double l2,
                                 double l3, double* R, double* t) {
    const PnpV3 x1 = psub(p1, p2), x2 = psub(p2, p3), x3 = pcross(x1, x2);
    const PnpV3 z1 = pscale(l1, y1), z2 = pscale(l2, y2), z3 = pscale(l3, y3);
    const PnpV3 u1 = psub(z1, z2), u2 = psub(z2, z3), u3 = pcross(u1, u2);
    const double det = pdot(x3, x3);  // det [x1 x2 x1 x x2]
    // rows of X^-1: (x2 x x3, x3 x x1, x1 x x2) / det
    const PnpV3 i1 = pscale(1.0 / det, pcross(x2, x3)), i2 = pscale(1.0 / det, pcross(x3, x1)),
                i3 = pscale(1.0 / det, x3);
    R[0] = (u1.x * i1.x + u2.x * i2.x) + u3.x * i3.x;
    R[1] = (u1.x * i1.y + u2.x * i2.y) + u3.x * i3.y;
    R[2] = (u1.x * i1.z + u2.x * i2.z) + u3.x * i3.z;
    R[3] = (u1.y * i1.x + u2.y * i2.x) + u3.y * i3.x;
    R[4] = (u1.y * i1.y + u2.y * i2.y) + u3.y * i3.y;
    R[5] = (u1.y * i1.z + u2.y * i2.z) + u3.y * i3.z;
    R[6] = (u1.z * i1.x + u2.z * i2.x) + u3.z * i3.x;
    R[7] = (u1.z * i1.y + u2.z * i2.y) + u3.z * i3.y;
    R[8] = (u1.z * i1.z + u2.z * i2.z) + u3.z * i3.z;
    t[0] = z1.x - ((R[0] * p1.x + R[1] * p1.y) + R[2] * p1.z);
    t[1] = z1.y - ((R[3] * p1.x + R[4] * p1.y) + R[5] * p1.z);
    t[2] = z1.z - ((R[6] * p1.x + R[7] * p1.y) + R[8] * p1.z);
    bool ok = pfinite3(pv(t[0], t[1], t[2]));
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && pfinite(R[k]);
    return ok;
}

// The depths on one line l . Lambda = 0 of the degenerate conic, cut with the pencil member Q: up to two depth
// triples appended to the pose list.  `emit` is a callable (l1, l2, l3) -> void.
template <class Emit>
PNP_HD void pnp_line_depths(const PnpTri& g, PnpS3 Q, PnpV3 l, Emit&& emit) {
    const double ax = pabs(l.x), ay = pabs(l.y), az = pabs(l.z);
    const int k = (az >= ax && az >= ay) ? 2 : (ay >= ax ? 1 : 0);  // the eliminated depth
    const double lk = k == 2 ? l.z : (k == 1 ? l.y : l.x);
    if (!(pabs(lk) > 0.0)) return;
    // Lambda = s (gv + tau hv), the other two depths in index order
    const double u = -(k == 0 ? l.y : l.x) / lk, v = -(k == 2 ? l.y : l.z) / lk;
    const PnpV3 gv = k == 2 ? pv(1.0, 0.0, u) : (k == 1 ? pv(1.0, u, 0.0) : pv(u, 1.0, 0.0));
    const PnpV3 hv = k == 2 ? pv(0.0, 1.0, v) : (k == 1 ? pv(0.0, v, 1.0) : pv(v, 0.0, 1.0));
    const PnpV3 Qg = smul(Q, gv), Qh = smul(Q, hv);
    const double A = pdot(hv, Qh), B = pdot(gv, Qh), C = pdot(gv, Qg);
    const double disc = B * B - A * C;
    if (!(disc >= 0.0)) return;
    const double sq = sqrt(disc);
    const double q = -(B + (B < 0.0 ? -sq : sq));
    const double tau1 = q / A, tau2 = C / q;
    const double asum = (g.a12 + g.a13) + g.a23;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const double tau = r == 0 ? tau1 : tau2;
        if (!(tau > 0.0) || !pfinite(tau)) continue;
        if (r == 1 && tau2 == tau1) continue;  // a double root once
        const PnpV3 w = padd(gv, pscale(tau, hv));
        // s^2 * (sum of the three constraint forms at w) = a12 + a13 + a23
        const double qf = (((w.x * w.x + w.y * w.y) - 2.0 * g.b12 * (w.x * w.y)) +
                           ((w.x * w.x + w.z * w.z) - 2.0 * g.b13 * (w.x * w.z))) +
                          ((w.y * w.y + w.z * w.z) - 2.0 * g.b23 * (w.y * w.z));
        if (!(qf > 0.0)) continue;
        const double s = sqrt(asum / qf);
        double l1 = s * w.x, l2 = s * w.y, l3 = s * w.z;
        if (!(l1 > 0.0 && l2 > 0.0 && l3 > 0.0)) continue;
        if (!pnp_polish(g, l1, l2, l3)) continue;
        emit(l1, l2, l3);
    }
}

// P3P on one sample: the pencil D1 + gamma D2 of the two homogeneous conics in the depths
// (D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23), one real root of its determinant's cubic, the degenerate
// member split into its two lines (adjugate method), each line cut with the pencil member farther from the
// degenerate one, every candidate polished on the three distance constraints.  y1..y3 are unit (f64-normalised).
template <class Emit>
PNP_HD void pnp_p3p_depths(const PnpTri& g, Emit&& emit) {
    const PnpS3 D1{g.a23, -g.a23 * g.b12, 0.0, g.a23 - g.a12, g.a12 * g.b23, -g.a12};
    const PnpS3 D2{g.a23, 0.0, -g.a23 * g.b13, -g.a13, g.a13 * g.b23, g.a23 - g.a13};
    const PnpV3 p0 = scol0(D1), p1 = scol1(D1), p2 = scol2(D1), q0 = scol0(D2), q1 = scol1(D2), q2 = scol2(D2);
    const double c3 = pdet(q0, q1, q2), c0 = pdet(p0, p1, p2);
    const double c2 = (pdet(p0, q1, q2) + pdet(q0, p1, q2)) + pdet(q0, q1, p2);
    const double c1 = (pdet(q0, p1, p2) + pdet(p0, q1, p2)) + pdet(p0, p1, q2);
    if (!(pabs(c3) > 0.0)) return;
    const double gamma = pnp_cubic_root(c2 / c3, c1 / c3, c0 / c3);
    if (!pfinite(gamma)) return;
    const PnpS3 D0 = saxpy(D1, gamma, D2);
    // B = -adj(D0) = p p^T with p the meeting point of the two lines
    const double B00 = -(D0.a11 * D0.a22 - D0.a12 * D0.a12), B11 = -(D0.a00 * D0.a22 - D0.a02 * D0.a02),
                 B22 = -(D0.a00 * D0.a11 - D0.a01 * D0.a01);
    const double B01 = D0.a01 * D0.a22 - D0.a02 * D0.a12, B02 = -(D0.a01 * D0.a12 - D0.a02 * D0.a11),
                 B12 = D0.a00 * D0.a12 - D0.a01 * D0.a02;
    const int sel = (B22 >= B00 && B22 >= B11) ? 2 : (B11 >= B00 ? 1 : 0);
    const double Bii = sel == 2 ? B22 : (sel == 1 ? B11 : B00);
    if (!(Bii > 0.0)) return;  // a complex line pair: no real intersection of the conics
    const double beta = sqrt(Bii);
    const PnpV3 pp = sel == 2 ? pv(B02 / beta, B12 / beta, B22 / beta)
                              : (sel == 1 ? pv(B01 / beta, B11 / beta, B12 / beta) : pv(B00 / beta, B01 / beta, B02 / beta));
    // C = D0 + [p]x = 2 m l^T: its rows are multiples of one line, its columns of the other
    const PnpV3 r0 = pv(D0.a00, D0.a01 - pp.z, D0.a02 + pp.y), r1 = pv(D0.a01 + pp.z, D0.a11, D0.a12 - pp.x),
                r2 = pv(D0.a02 - pp.y, D0.a12 + pp.x, D0.a22);
    const double n0 = pdot(r0, r0), n1 = pdot(r1, r1), n2 = pdot(r2, r2);
    const PnpV3 la = (n2 >= n0 && n2 >= n1) ? r2 : (n1 >= n0 ? r1 : r0);
    const PnpV3 k0 = pv(r0.x, r1.x, r2.x), k1 = pv(r0.y, r1.y, r2.y), k2 = pv(r0.z, r1.z, r2.z);
    const double m0 = pdot(k0, k0), m1 = pdot(k1, k1), m2 = pdot(k2, k2);
    const PnpV3 lb = (m2 >= m0 && m2 >= m1) ? k2 : (m1 >= m0 ? k1 : k0);
    const bool useD2 = pabs(gamma) < 1.0;
    const PnpS3 Q = useD2 ? D2 : D1;
    pnp_line_depths(g, Q, la, emit);
    pnp_line_depths(g, Q, lb, emit);
}

// known rotation: (I - b b^T)(a + t) = 0 for two points (b unit), N t = -sum (I - b b^T) a, by the adjugate of
// the symmetric N.  False when N is singular, t is not finite, or a sampled point ends up behind the camera.
PNP_HD bool pnp_known_rotation(PnpV3 a1, PnpV3 y1, PnpV3 a2, PnpV3 y2, double* t) {
    const PnpS3 N{(1.0 - y1.x * y1.x) + (1.0 - y2.x * y2.x), -(y1.x * y1.y) - y2.x * y2.y, -(y1.x * y1.z) - y2.x * y2.z,
                  (1.0 - y1.y * y1.y) + (1.0 - y2.y * y2.y), -(y1.y * y1.z) - y2.y * y2.z,
                  (1.0 - y1.z * y1.z) + (1.0 - y2.z * y2.z)};
    const PnpV3 s1 = psub(a1, pscale(pdot(y1, a1), y1)), s2 = psub(a2, pscale(pdot(y2, a2), y2));
    const PnpV3 rhs = pv(-(s1.x + s2.x), -(s1.y + s2.y), -(s1.z + s2.z));
    const PnpV3 c0 = scol0(N), c1 = scol1(N), c2 = scol2(N);
    const double det = pdet(c0, c1, c2);
    if (!(det > 0.0)) return false;
    t[0] = pdet(rhs, c1, c2) / det;
    t[1] = pdet(c0, rhs, c2) / det;
    t[2] = pdet(c0, c1, rhs) / det;
    const PnpV3 tv = pv(t[0], t[1], t[2]);
    return pfinite3(tv) && pdot(y1, padd(a1, tv)) > 0.0 && pdot(y2, padd(a2, tv)) > 0.0;
}

PNP_HD PnpV3 pnp_load3(const float* a, int i) {
    return pv((double)a[3 * i], (double)a[3 * i + 1], (double)a[3 * i + 2]);
}

// One sample row: the skip predicates, then the minimal solver.  Writes the row's poses (R 9, t 3 each, at most
// four) to `out` and returns their number; 0: the row is skipped.  k is not read in mode B (known rotation Rk).
PNP_HD int pnp_row_poses(const float* points, const float* bearings, int i, int j, int k, bool known, const double* Rk,
                         double cp2, double* out) {
    int nsol = 0;
    const PnpV3 p1 = pnp_load3(points, i), p2 = pnp_load3(points, j), b1 = pnp_load3(bearings, i),
                b2 = pnp_load3(bearings, j);
    bool ok = i != j && pfinite3(p1) && pfinite3(p2) && pfinite3(b1) && pfinite3(b2) && !pnp_pair_close(b1, b2, cp2);
    const double n1 = pdot(b1, b1), n2 = pdot(b2, b2);
    ok = ok && n1 > 0.0 && n2 > 0.0;
    if (known) {
        if (!ok) return 0;
        const PnpV3 y1 = pscale(1.0 / sqrt(n1), b1), y2 = pscale(1.0 / sqrt(n2), b2);
        const double zero[3] = {0.0, 0.0, 0.0};
        double t[3];
        if (!pnp_known_rotation(pnp_transform(Rk, zero, p1), y1, pnp_transform(Rk, zero, p2), y2, t)) return 0;
#pragma unroll
        for (int q = 0; q < 9; ++q) out[q] = Rk[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) out[9 + q] = t[q];
        return 1;
    }
    const PnpV3 p3 = pnp_load3(points, k), b3 = pnp_load3(bearings, k);
    const double n3 = pdot(b3, b3);
    ok = ok && i != k && j != k && pfinite3(p3) && pfinite3(b3) && n3 > 0.0 && !pnp_pair_close(b1, b3, cp2) &&
         !pnp_pair_close(b2, b3, cp2) && !pnp_collinear(p1, p2, p3);
    if (!ok) return 0;
    const PnpV3 y1 = pscale(1.0 / sqrt(n1), b1), y2 = pscale(1.0 / sqrt(n2), b2), y3 = pscale(1.0 / sqrt(n3), b3);
    const PnpV3 e12 = psub(p1, p2), e13 = psub(p1, p3), e23 = psub(p2, p3);
    const PnpTri g{pdot(e12, e12), pdot(e13, e13), pdot(e23, e23), pdot(y1, y2), pdot(y1, y3), pdot(y2, y3)};
    pnp_p3p_depths(g, [&](double l1, double l2, double l3) {
        if (nsol >= 4) return;
        double R[9], t[3];
        if (!pnp_pose_from_depths(p1, p2, p3, y1, y2, y3, l1, l2, l3, R, t)) return;
        double* o = out + 12 * nsol;
#pragma unroll
        for (int q = 0; q < 9; ++q) o[q] = R[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) o[9 + q] = t[q];
        ++nsol;
    });
    return nsol;
}

}  // namespace vio360
