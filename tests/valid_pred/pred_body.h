// pred_body.h — TEST TOOLING: the cases of pred_equiv.cpp for ONE precision.  Included once per
// precision, inside a namespace of its own, right after rt_trace.h of the same RT_F64.  Every case
// prints one line: family, index, decision, the bits of t (and of what else the test returns), and
// whether one of the operands a validity rule reads (t, a, b; the box's entry and exit) is a NaN.
// isect_plane<1> is called as the flat loops call it; test_box<true> is the flat loops' form and
// test_box<false> the BVH surface prefix's, which keeps the margins in both builds.
using namespace RT_NS;

#if RT_F64
#define PV_PREC "f64"
static unsigned long long bits(real x) { return __builtin_bit_cast(unsigned long long, x); }
#else
#define PV_PREC "f32"
static unsigned long long bits(real x) { return __builtin_bit_cast(uint32_t, x); }
#endif
static real up(real x) { return std::nextafter(x, (real)HUGE_VAL); }
static real dn(real x) { return std::nextafter(x, -(real)HUGE_VAL); }
static bool is_nan(real x) { return x != x; }

// ---------------------------------------------------------------- random numbers (splitmix64)
struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  double uni(double a, double b) { return a + (b - a) * (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};
struct D3 {
  double x, y, z;
};
static D3 cross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static double dotd(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static D3 scale(double s, D3 a) { return D3{s * a.x, s * a.y, s * a.z}; }
static D3 add(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
static D3 unitd(D3 a) { return scale(1.0 / std::sqrt(dotd(a, a)), a); }
static D3 rand_unit(Rng& g) {
  for (;;) {
    D3 v{g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)};
    const double l = dotd(v, v);
    if (l > 0.01 && l <= 1.0) return unitd(v);
  }
}
static f3 to3(D3 a) { return f3{(real)a.x, (real)a.y, (real)a.z}; }

// ---------------------------------------------------------------- parallelograms
// the record of the parallelogram (q, u, v) with unit normal n: a = n, b = q, c = wa, e = wb
static PrimRec plane_rec(D3 n, D3 q, D3 u, D3 v) {
  const D3 cp = cross(u, v);
  const D3 ns = scale(1.0 / std::sqrt(dotd(cp, cp)), n);
  const D3 wa = cross(v, ns), wb = cross(ns, u);
  PrimRec r{};
  r.a = v4{(real)n.x, (real)n.y, (real)n.z, 0};
  r.b = v4{(real)q.x, (real)q.y, (real)q.z, 0};
  r.c = v4{(real)wa.x, (real)wa.y, (real)wa.z, 0};
  r.e = v4{(real)wb.x, (real)wb.y, (real)wb.z, 0};
  return r;
}
static long long plane_index = 0;
// isect_plane<1> without and with the target term; `consider` on a ray without a hit so far
static void plane_case(const char* fam, const PrimRec& r, f3 o, f3 d, real tmin, bool self) {
  RayCtx R{};
  R.o = o, R.d = d;
  const real tu = float_up(tmin);
  // the operands the rules read, by isect_plane's own arithmetic (only to mark the NaN cases)
  const real denom = dot(xyz(r.a), d);
  const f3 qo = xyz(r.b) - o;
  const real tt = dot(xyz(r.a), qo) * RT_RCP_NZ(denom);
  const f3 prel = tt * d - qo;
  const real aa = dot(prel, xyz(r.c)), bb = dot(prel, xyz(r.e));
  const int nan = is_nan(tt) || is_nan(aa) || is_nan(bb) || is_nan(denom);
  for (int with_tgt = 0; with_tgt < 2; ++with_tgt) {
    real t = RT_NAN, q = -RL(1.0), tg = -RL(7.0);
    isect_plane<1>(r, o, R, tu, self, t, q, false, with_tgt ? &tg : nullptr);
    Closest C = no_hit();
    consider<false>(C, t, q, 1, 7);
    std::printf("%s %s tgt%d %lld dec=%d take=%d t=%llx tg=%llx nan=%d\n", PV_PREC, fam, with_tgt, plane_index,
                q >= RL(0.0) ? 1 : 0, C.prim == 7 ? 1 : 0, bits(t), bits(tg), nan);
  }
  ++plane_index;
}

static void plane_cases() {
  const real tm = kTmin;
  // unit square in z = 0, dyadic edges: a = x and b = y of the hit point, exactly
  const PrimRec unit = plane_rec(D3{0, 0, 1}, D3{0, 0, 0}, D3{1, 0, 0}, D3{0, 1, 0});
  // a, b at 0 and 1 and one ulp (the smallest denormal at 0) to each side, all pairs
  const real edge[] = {RL(0.0), -RL(0.0), up(RL(0.0)), dn(RL(0.0)), RL(1.0), up(RL(1.0)), dn(RL(1.0)), RL(0.5),
                       RL(1e-30), -RL(1e-30)};
  for (real a : edge)
    for (real b : edge)
      for (int self = 0; self < 2; ++self) plane_case("ab_edge", unit, f3{a, b, RL(1.0)}, f3{0, 0, -RL(1.0)}, tm, self != 0);
  // t at tmin_up and one ulp to each side (axis-aligned ray: t is exact), for several tmin
  for (real tmin : {kTmin, RL(0.5), RL(1e-30), RL(3.0)}) {
    const real tu = float_up(tmin);
    for (real T : {tmin, tu, up(tu), dn(tmin), RL(0.0), -tu}) {
      const PrimRec r = plane_rec(D3{0, 0, 1}, D3{0, 0, (double)T}, D3{4, 0, 0}, D3{0, 4, 0});
      plane_case("t_edge", r, f3{RL(0.25), RL(0.25), 0}, f3{0, 0, RL(1.0)}, tmin, false);
    }
  }
  // |n . d| at 1e-8 and one ulp to each side, both signs, and zero (n . d = delta exactly)
  {
    const PrimRec r = plane_rec(D3{0, 0, 1}, D3{0, 0, 0}, D3{4, 0, 0}, D3{0, 4, 0});
    const real e = RL(1e-8);
    for (real dl : {e, up(e), dn(e), -e, -up(e), -dn(e), RL(0.0), -RL(0.0), RL(1e-30), -RL(1e-30)})
      plane_case("denom_edge", r, f3{RL(0.25), RL(0.25), -dl}, f3{RL(1.0), 0, dl}, tm, false);
  }
  // the target term's own rules: t in (0, tmin_up) is a target hit and no candidate
  for (real T : {RL(0.0), up(RL(0.0)), RL(1e-6), tm, float_up(tm), -RL(1e-6)}) {
    const PrimRec r = plane_rec(D3{0, 0, 1}, D3{0, 0, (double)T}, D3{4, 0, 0}, D3{0, 4, 0});
    plane_case("target_t", r, f3{RL(0.25), RL(0.25), 0}, f3{0, 0, RL(1.0)}, tm, false);
    plane_case("target_t", r, f3{RL(0.25), RL(0.25), 0}, f3{0, 0, RL(1.0)}, tm, true);
  }
  // operands that are not finite
  {
    const real bad[] = {RT_NAN, RT_HUGE, -RT_HUGE};
    for (real v : bad)
      for (int k = 0; k < 6; ++k) {
        real od[6] = {RL(0.25), RL(0.25), RL(1.0), RL(0.6), 0, -RL(0.8)};
        od[k] = v;
        plane_case("non_finite", unit, f3{od[0], od[1], od[2]}, f3{od[3], od[4], od[5]}, tm, false);
      }
    PrimRec r = unit;
    r.c.x = RT_NAN;
    plane_case("non_finite", r, f3{RL(0.25), RL(0.25), RL(1.0)}, f3{0, 0, -RL(1.0)}, tm, false);
    r = unit;
    r.b.z = RT_HUGE;
    plane_case("non_finite", r, f3{RL(0.25), RL(0.25), RL(1.0)}, f3{0, 0, -RL(1.0)}, tm, false);
  }
  // 2^16 random well-conditioned cases: a third hit, a third missed, a third within 1e-3 of an edge
  Rng g{20240611};
  for (int i = 0; i < 65536; ++i) {
    const D3 n = rand_unit(g);
    const D3 u = scale(g.uni(0.5, 4), unitd(cross(n, rand_unit(g))));
    const D3 v = scale(g.uni(0.5, 4), unitd(add(cross(n, unitd(u)), scale(g.uni(-0.5, 0.5), unitd(u)))));
    const D3 q{g.uni(-2, 2), g.uni(-2, 2), g.uni(-2, 2)};
    double a, b;
    switch (i % 3) {
      case 0: a = g.uni(0.01, 0.99), b = g.uni(0.01, 0.99); break;
      case 1: a = g.uni(1.01, 2) * (g.next() & 1 ? 1 : -1), b = g.uni(-1, 2); break;
      default: a = (g.next() & 1 ? 1.0 : 0.0) + g.uni(-1e-3, 1e-3), b = g.uni(0, 1); break;
    }
    const D3 p = add(q, add(scale(a, u), scale(b, v)));
    D3 d = rand_unit(g);
    if (std::fabs(dotd(d, n)) < 0.05) d = unitd(add(d, n));
    const double t = i % 7 == 6 ? -g.uni(0.1, 5) : g.uni(0.1, 5);
    const D3 o = add(p, scale(-t, d));
    plane_case("random", plane_rec(n, q, u, v), to3(o), to3(d), tm, i % 11 == 0);
  }
}

// ---------------------------------------------------------------- box groups
// the record of the box with corner c, unit axes e_k and edge lengths L_k.  Face f = 2 axis + side has
// key order 10 + f, gid 20 + f and primitive 40 + f; `missing`: a face the box does not have
struct Box {
  RT_NS::DevBox B;
  D3 c, e[3];
  double L[3];
};
static Box make_box(D3 c, const D3 e[3], const double L[3], int missing) {
  Box X{};
  X.c = c;
  for (int k = 0; k < 3; ++k) {
    X.e[k] = e[k], X.L[k] = L[k];
    const D3 a = scale(1.0 / L[k], e[k]);
    real* dst = k == 0 ? X.B.a0 : k == 1 ? X.B.a1 : X.B.a2;
    dst[0] = (real)a.x, dst[1] = (real)a.y, dst[2] = (real)a.z;
    X.B.sc[k] = (real)dotd(a, c);
  }
  int code = 0;
  for (int f = 0; f < 6; ++f) code |= (f == missing ? RT_BOX_NO_FACE : f) << (5 * f);
  X.B.ord_base = 10, X.B.gid_base = 20, X.B.prim_base = 40;
  X.B.ord_code = X.B.gid_code = X.B.prim_code = code;
  return X;
}
static D3 rot_y(D3 v, double deg) {
  const double a = deg * 3.14159265358979323846 / 180, c = std::cos(a), s = std::sin(a);
  return D3{c * v.x + s * v.z, v.y, -s * v.x + c * v.z};
}
static D3 rot_x(D3 v, double deg) {
  const double a = deg * 3.14159265358979323846 / 180, c = std::cos(a), s = std::sin(a);
  return D3{v.x, c * v.y - s * v.z, s * v.y + c * v.z};
}
// world point / direction of box-frame coordinates s (s_k in [0, 1] inside)
static D3 box_point(const Box& X, D3 s) {
  return add(X.c, add(scale(s.x * X.L[0], X.e[0]), add(scale(s.y * X.L[1], X.e[1]), scale(s.z * X.L[2], X.e[2]))));
}
static D3 box_dir(const Box& X, D3 s) {
  return add(scale(s.x * X.L[0], X.e[0]), add(scale(s.y * X.L[1], X.e[1]), scale(s.z * X.L[2], X.e[2])));
}
static long long box_index = 0;
template <bool kKeyOnly>
static void box_run(const char* fam, const char* rec, const Box& X, const RayCtx& R, real tu, int nan) {
  Closest C = no_hit();
  test_box<kKeyOnly>((const RT_CAS RT_NS::DevBox*)&X.B, R, tu, C);
#if RT_F64
  const unsigned long long tb = bits(C.t);
  const int ord = C.t < kInf ? C.ord : -1;
#else
  const unsigned long long tb = kKeyOnly ? C.key >> 32 : bits(C.t);
  const int ord = kKeyOnly ? (C.key == no_hit().key ? -1 : (int)(unsigned)(C.key & 0xffffffffull)) : -1;
#endif
  const int dec = kKeyOnly ? ord >= 0 : C.prim >= 0;
  std::printf("%s box_%s %s key%d %lld dec=%d t=%llx ord=%d prim=%d nan=%d\n", PV_PREC, fam, rec, kKeyOnly ? 1 : 0,
              box_index, dec, tb, kKeyOnly ? ord : 0, kKeyOnly ? 0 : C.prim, nan);
}
static void box_case(const char* fam, const char* rec, const Box& X, f3 o, f3 d, real tmin, int self_gid) {
  RayCtx R{};
  R.o = o, R.d = d, R.self_gid = self_gid, R.self_inst = -1;
  // the slab entry and exit by test_box's own arithmetic (only to mark the NaN cases)
  const f3 ax[3] = {f3{X.B.a0[0], X.B.a0[1], X.B.a0[2]}, f3{X.B.a1[0], X.B.a1[1], X.B.a1[2]},
                    f3{X.B.a2[0], X.B.a2[1], X.B.a2[2]}};
  real inv[3], lo[3], hi[3];
#if RT_F64 && !defined(RT_BOX_THREE_RCP)
  {
    real dk[3];
    for (int k = 0; k < 3; ++k) dk[k] = dot(ax[k], d);
    const real d01 = dk[0] * dk[1], p = d01 * dk[2];
    const real r = RT_RCP_NZ(p);
    inv[0] = r * (dk[1] * dk[2]), inv[1] = r * (dk[0] * dk[2]), inv[2] = r * d01;
    if (!(RABS(p) >= RL(1e-300) && RABS(p) <= RL(1e300)))
      for (int k = 0; k < 3; ++k) inv[k] = box_rcp(dk[k]);
  }
#else
  for (int k = 0; k < 3; ++k) inv[k] = box_rcp(dot(ax[k], d));
#endif
  for (int k = 0; k < 3; ++k) {
    const real s = RFMA(ax[k].x, o.x, RFMA(ax[k].y, o.y, RFMA(ax[k].z, o.z, -X.B.sc[k])));
    const real t0 = -s * inv[k], t1 = RFMA(-s, inv[k], inv[k]);
    lo[k] = RMIN(t0, t1), hi[k] = RMAX(t0, t1);
  }
  const real tn = RMAX(RMAX(lo[0], lo[1]), lo[2]), tf = RMIN(RMIN(hi[0], hi[1]), hi[2]);
  const int nan = is_nan(tn) || is_nan(tf);
  const real tu = float_up(tmin);
  box_run<true>(fam, rec, X, R, tu, nan);
  box_run<false>(fam, rec, X, R, tu, nan);
  ++box_index;
}

static void box_cases() {
  const D3 ex[3] = {D3{1, 0, 0}, D3{0, 1, 0}, D3{0, 0, 1}};
  const double unitL[3] = {1, 1, 1};
  const Box unit = make_box(D3{0, 0, 0}, ex, unitL, -1);  // dyadic: its slab ends are exact
  const real tm = kTmin;
  // tf == tn (a ray through the edge x = 1, y = 0 of the unit box) and one ulp to each side; the z
  // axis is parallel to the ray (+0 and -0)
  for (real oy : {-RL(2.0), up(-RL(2.0)), dn(-RL(2.0))})
    for (real dz : {RL(0.0), -RL(0.0)})
      for (real oz : {RL(0.5), RL(0.0), RL(1.0), RL(1.5)})
        box_case("edge", "unit", unit, f3{-RL(1.0), oy, oz}, f3{RL(1.0), RL(1.0), dz}, tm, -1);
  // the entry and the exit at tmin_up and one ulp to each side (rays along x: t is exact)
  for (real tmin : {kTmin, RL(0.5), RL(1e-30)}) {
    const real tu = float_up(tmin);
    for (real T : {tmin, tu, up(tu), dn(tmin)}) {
      box_case("t_entry", "unit", unit, f3{-T, RL(0.5), RL(0.5)}, f3{RL(1.0), 0, 0}, tmin, -1);
      box_case("t_exit", "unit", unit, f3{RL(1.0) - T, RL(0.5), RL(0.5)}, f3{RL(1.0), 0, 0}, tmin, -1);
      box_case("t_exit", "unit", unit, f3{T, RL(0.5), RL(0.5)}, f3{-RL(1.0), -RL(0.0), RL(0.0)}, tmin, -1);
    }
  }
  // slabs whose ends overflow to infinities of one sign: an axis parallel to the ray, far outside
  for (real far : {RL(1e30), -RL(1e30)})
    for (real z : {RL(0.0), -RL(0.0)}) {
      box_case("overflow", "unit", unit, f3{-RL(1.0), far, RL(0.5)}, f3{RL(1.0), z, z}, tm, -1);
      box_case("overflow", "unit", unit, f3{RL(0.5), far, far}, f3{RL(1.0), z, -z}, tm, -1);
      box_case("overflow", "unit", unit, f3{far, far, far}, f3{z, z, RL(1.0)}, tm, -1);
    }
  // operands that are not finite
  for (real v : {RT_NAN, RT_HUGE, -RT_HUGE})
    for (int k = 0; k < 6; ++k) {
      real od[6] = {-RL(1.0), RL(0.5), RL(0.25), RL(0.8), RL(0.1), RL(0.05)};
      od[k] = v;
      box_case("non_finite", "unit", unit, f3{od[0], od[1], od[2]}, f3{od[3], od[4], od[5]}, tm, -1);
    }
  // the four records: axis-aligned, rotated about y (the Cornell boxes), doubly rotated, and the
  // room: a box seen from inside that lacks the face the camera looks through
  D3 ry[3], rxy[3];
  for (int k = 0; k < 3; ++k) ry[k] = rot_y(ex[k], 15), rxy[k] = rot_x(rot_y(ex[k], -18), 31);
  const double La[3] = {165, 330, 165}, Lr[3] = {555, 555, 555};
  const Box recs[4] = {make_box(D3{130, 0, 65}, ex, La, -1), make_box(D3{265, 0, 295}, ry, La, -1),
                       make_box(D3{-40, 25, 10}, rxy, La, -1), make_box(D3{0, 0, 0}, ex, Lr, 4)};
  const char* names[4] = {"aligned", "rot_y", "rot_xy", "room"};
  Rng g{977};
  for (int b = 0; b < 4; ++b) {
    const Box& X = recs[b];
    // rays parallel to one axis and to two axes of the box, +0 and -0 components, from inside, from a
    // face (leaving it: self) and from outside
    const double zs[2] = {0.0, -0.0};
    for (int ax = 0; ax < 3; ++ax)
      for (int two = 0; two < 2; ++two)
        for (int sg = 0; sg < 4; ++sg)
          for (int where = 0; where < 4; ++where) {
            double s[3] = {zs[sg & 1], zs[sg >> 1], zs[(sg ^ (sg >> 1)) & 1]};
            s[ax] = sg & 1 ? -1.0 : 1.0;
            if (!two) s[(ax + 1) % 3] = sg & 2 ? -0.7 : 0.4;
            double p[3] = {0.3, 0.6, 0.45};
            int self = -1;
            if (where == 1) p[ax] = -1.5;                       // outside, before the box
            if (where == 2) p[ax] = 2.5;                        // outside, behind it
            if (where == 3) p[ax] = s[ax] > 0 ? 0.0 : 1.0, self = 20 + 2 * ax + (s[ax] > 0 ? 0 : 1);  // on a face
            // axis-aligned records: the direction is exactly parallel (the zero components stay zeros)
            const D3 dw = b == 0 || b == 3 ? D3{s[0], s[1], s[2]} : unitd(box_dir(X, D3{s[0] / X.L[0], s[1] / X.L[1], s[2] / X.L[2]}));
            box_case("parallel", names[b], X, to3(box_point(X, D3{p[0], p[1], p[2]})), to3(dw), tm, self);
          }
    // random well-conditioned rays, 2^14 per record: origins inside, on a face and outside
    for (int i = 0; i < 16384; ++i) {
      D3 s{g.uni(0.02, 0.98), g.uni(0.02, 0.98), g.uni(0.02, 0.98)};
      int self = -1;
      const int where = i % 4;
      if (where == 1) {
        const int f = (int)(g.next() % 6);
        double* sk = f / 2 == 0 ? &s.x : f / 2 == 1 ? &s.y : &s.z;
        *sk = f & 1 ? 1.0 : 0.0;
        self = 20 + f;
      } else if (where >= 2) {
        s = D3{g.uni(-2, 3), g.uni(-2, 3), g.uni(-2, 3)};
      }
      const D3 o = box_point(X, s);
      // outside origins aim at a point of the box three times out of four
      D3 d = rand_unit(g);
      if (where >= 2 && i % 16 >= 4) {
        const D3 aim = box_point(X, D3{g.uni(0, 1), g.uni(0, 1), g.uni(0, 1)});
        d = unitd(add(aim, scale(-1, o)));
      }
      box_case("random", names[b], X, to3(o), to3(d), tm, self);
    }
  }
}

static void run_all() {
  plane_cases();
  box_cases();
}
#undef PV_PREC
