// cull_body.h — TEST TOOLING: the checks of cull_rects.cpp for ONE precision.  Included once per
// precision, inside a namespace of its own, right after rt_trace.h of the same RT_F64.
// For every box group and static parallelogram of the flat surface set that has a screen rectangle
// (KernelParams::cull_box / cull_quad) the frame is swept: through every pixel's footprint 20
// camera rays (its four corners and 16 jittered points), made as camera_ray_flat makes them, are
// tested against the record alone with the flat loops' own tests (test_box<true>,
// test_static<RT_PRIM_CLASS_QUAD>).  One line per record; a line that starts with FAIL fails the test.
using namespace RT_NS;
using KP = RT_NS::KernelParams;  // (the global alias is the FP32 one)

#if RT_F64
#define PC_PREC "f64"
static bool candidate(const Closest& C) { return C.t < kInf; }
#else
#define PC_PREC "f32"
static bool candidate(const Closest& C) { return (uint32_t)(C.key >> 32) < 0x7f800000u; }
#endif

struct Dv {
  double x, y, z;
};
static Dv sub(Dv a, Dv b) { return Dv{a.x - b.x, a.y - b.y, a.z - b.z}; }
static Dv add(Dv a, Dv b) { return Dv{a.x + b.x, a.y + b.y, a.z + b.z}; }
static Dv mul(double s, Dv a) { return Dv{s * a.x, s * a.y, s * a.z}; }
static double dotv(Dv a, Dv b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static Dv crossv(Dv a, Dv b) { return Dv{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static Dv dv(const real* p) { return Dv{(double)p[0], (double)p[1], (double)p[2]}; }

static RayCtx camera_ray_at(const KP& P, double a, double b) {
  RayCtx R{};
  const f3 origin = ld3(P.cam.center);
  const f3 target = ld3(P.cam.top_left) + (real)a * ld3(P.cam.pixel_u) + (real)b * ld3(P.cam.pixel_v);
  R.o = origin;
  R.d = normalize(target - origin);
  R.self_gid = -1;
  R.self_inst = -1;
  return R;
}

struct Sweep {
  int x0, x1, y0, y1;  // the tight rectangle of the pixels with a valid candidate (x0 > x1: none)
  int outside_hits;    // pixels outside the record's rectangle with a valid candidate
};
template <class Test>
static Sweep sweep(const KP& P, const uint32_t* rect, Test test) {
  const int W = P.cam.width, H = P.cam.height;
  const int rx0 = (int)(rect[0] & 0xffffu), rx1 = (int)(rect[1] & 0xffffu), ry0 = (int)(rect[0] >> 16), ry1 = (int)(rect[1] >> 16);
  Sweep S{W, -1, H, -1, 0};
  uint64_t s = 0x1234567ull;
  auto uni = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);
  };
  for (int gy = 0; gy < H; ++gy)
    for (int px = 0; px < W; ++px) {
      bool any = false;
      for (int k = 0; k < 20 && !any; ++k) {
        const double a = k < 4 ? px + (k & 1) : px + uni(), b = k < 4 ? gy + (k >> 1) : gy + uni();
        const RayCtx R = camera_ray_at(P, a, b);
        Closest C = no_hit();
        test(R, C);
        any = candidate(C);
      }
      if (!any) continue;
      S.x0 = std::min(S.x0, px), S.x1 = std::max(S.x1, px), S.y0 = std::min(S.y0, gy), S.y1 = std::max(S.y1, gy);
      if (px < rx0 || px > rx1 || gy < ry0 || gy > ry1) ++S.outside_hits;
    }
  return S;
}

// One record's line.  corners: the record's corners, by formulas of this file's own
static int report(const KP& P, const char* kind, int j, const uint32_t* rect, const Dv* corners, int n,
                  const Sweep& S) {
  const int W = P.cam.width, H = P.cam.height;
  const Dv c = dv(P.cam.center);
  const Dv fwd = sub(add(dv(P.cam.top_left), add(mul(0.5 * W, dv(P.cam.pixel_u)), mul(0.5 * H, dv(P.cam.pixel_v)))), c);
  bool behind = false;
  for (int i = 0; i < n; ++i) behind = behind || !(dotv(sub(corners[i], c), fwd) > 0);
  const bool want_all = P.cam_defocus || behind;
  const bool all = rect[0] == 0u && rect[1] == 0xffffffffu;
  // the rectangle cut to the frame, against the tight one
  const int rx0 = std::max(0, (int)(rect[0] & 0xffffu)), rx1 = std::min(W - 1, (int)(rect[1] & 0xffffu));
  const int ry0 = std::max(0, (int)(rect[0] >> 16)), ry1 = std::min(H - 1, (int)(rect[1] >> 16));
  const bool seen = S.x0 <= S.x1, on_frame = rx0 <= rx1 && ry0 <= ry1;
  bool ok = S.outside_hits == 0 && all == want_all;
  if (!all) {
    if (seen)
      ok = ok && on_frame && std::abs(rx0 - S.x0) <= 2 && std::abs(rx1 - S.x1) <= 2 && std::abs(ry0 - S.y0) <= 2 &&
           std::abs(ry1 - S.y1) <= 2;
    else  // nothing of it on the frame: at most the padding reaches in
      ok = ok && (!on_frame || (rx1 - rx0 <= 1 || ry1 - ry0 <= 1));
  }
  std::printf("%s %s %s %d all=%d want_all=%d rect=%d..%d,%d..%d tight=%d..%d,%d..%d outside_hits=%d\n", ok ? "ok" : "FAIL",
              PC_PREC, kind, j, all ? 1 : 0, want_all ? 1 : 0, rx0, rx1, ry0, ry1, S.x0, S.x1, S.y0, S.y1, S.outside_hits);
  return ok ? 0 : 1;
}

static int run(const HostScene& H, const rt_camera_settings& cs) {
  KP P;
  std::string err;
  rt_exec ex{};
  ex.n_shards = 1, ex.row_block = 4;
  const int variant = rt_host_variant(H);
  if (rt_host_render_params(H, variant, rt_host_records<real>(H), &cs, 1234u, &ex, LaunchInputs{}, P, err) != RT_OK) {
    std::printf("FAIL %s params: %s\n", PC_PREC, err.c_str());
    return 1;
  }
  const HostArraysT<real>& A = H.arrays<real>();
  const DevFlatSet& S = P.flat_sets[0];
  const real tmin_up = float_up(kTmin);
  int bad = 0, n = 0;
  for (int b = S.box_first; b < S.box_end && b - S.box_first < RT_CULL_BOXES; ++b, ++n) {
    const DevBoxT<real>& B = A.boxes[b];
    // a rectangular box: orthogonal axes a_k = e_k / L_k, so p = sum_k (s_k + sc_k) a_k / |a_k|^2
    const Dv ax[3] = {dv(B.a0), dv(B.a1), dv(B.a2)};
    Dv c[8];
    for (int i = 0; i < 8; ++i) {
      c[i] = Dv{0, 0, 0};
      for (int k = 0; k < 3; ++k) c[i] = add(c[i], mul(((double)B.sc[k] + (i >> k & 1)) / dotv(ax[k], ax[k]), ax[k]));
    }
    const uint32_t* rect = P.cull_box[b - S.box_first];
    const Sweep W = sweep(P, rect, [&](const RayCtx& R, Closest& C) { test_box<true>(&B, R, tmin_up, C); });
    bad += report(P, "box", b - S.box_first, rect, c, 8, W);
  }
  for (int k = S.first; k < S.end_quad && k - S.first < RT_CULL_QUADS; ++k, ++n) {
    const real* f = A.flat_recs.data() + 16 * (size_t)k;
    // u is normal to wb and n with wa . u = 1; v is normal to n and wa with wb . v = 1
    const Dv nn = dv(f), q = dv(f + 4), wa = dv(f + 8), wb = dv(f + 12);
    const Dv u0 = crossv(wb, nn), v0 = crossv(nn, wa);
    const Dv u = mul(1.0 / dotv(wa, u0), u0), v = mul(1.0 / dotv(wb, v0), v0);
    const Dv c[4] = {q, add(q, u), add(q, v), add(add(q, u), v)};
    const uint32_t* rect = P.cull_quad[k - S.first];
    const PrimRec rec = ld_rec64((const PrimRec64*)f);
    const Sweep W = sweep(P, rect, [&](const RayCtx& R, Closest& C) {
      test_static<RT_PRIM_CLASS_QUAD>(rec, R, kTmin, tmin_up, C);
    });
    bad += report(P, "quad", k - S.first, rect, c, 4, W);
  }
  std::printf("%s %s records=%d flat=%d\n", n > 0 && H.flat ? "ok" : "FAIL", PC_PREC, n, H.flat ? 1 : 0);
  return bad + (n > 0 && H.flat ? 0 : 1);
}
