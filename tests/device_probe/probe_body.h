// probe_body.h — TEST TOOLING: element-wise probes of rt_trace.h's own functions for ONE precision.
// Included once per precision, inside a namespace of its own, right after rt_trace.h of the same
// RT_F64 (the per-precision macros RT_RCP, RT_LOG, ... are those of the last include), by
// tests/device_probe/rt_probe.hip (gfx950) and tests/kernel_emu/rt_emu.cpp (host).  The includer
// defines RT_PROBE_DEFINE(name, params, args), which turns one entry of the lists at the end into
// an entry point over n elements: element i is pb_<name>(i, args...).  Every probe reads and
// writes element i of plain arrays only; nothing here is linked into librt_amd.so.
using namespace RT_NS;

// op: 0 RT_RCP, 1 RT_RCP_NZ, 2 RT_SQRT, 3 RT_RSQRT, 4 RT_LOG
RT_FN void pb_math1(int i, int op, const real* x, real* y) {
  const real v = x[i];
  real r = v;
  switch (op) {
    case 0: r = RT_RCP(v); break;
    case 1: r = RT_RCP_NZ(v); break;
    case 2: r = RT_SQRT(v); break;
    case 3: r = RT_RSQRT(v); break;
    case 4: r = RT_LOG(v); break;
  }
  y[i] = r;
}
// the kernel's uses of a uniform: op 0 u01(w), 1 1 - u01(w), 2 RT_LOG(1 - u01(w)) (medium_draw),
// 3 RT_SQRT(u01(w)) (the cosine and cone samplers)
RT_FN void pb_uniform(int i, int op, const uint32_t* w, real* y) {
  const real u = u01(w[i]);
  real r = u;
  switch (op) {
    case 1: r = RL(1.0) - u; break;
    case 2: r = RT_LOG(RL(1.0) - u); break;
    case 3: r = RT_SQRT(u); break;
  }
  y[i] = r;
}
// binary64: rt_math64::sincos_turns itself on both sides (the device's RT_SINCOS_TURNS; the host
// emulator's macro is libm's sin / cos of fl(2 pi) u, whose argument rounding alone is 3 2^-52)
RT_FN void pb_sincos(int i, const uint32_t* w, real* s, real* c) {
  real sn, cs;
#if RT_F64
  rt_math64::sincos_turns(u01(w[i]), &sn, &cs);
#else
  RT_SINCOS_TURNS(u01(w[i]), &sn, &cs);
#endif
  s[i] = sn;
  c[i] = cs;
}
RT_FN void pb_unit_vector(int i, const uint32_t* a, const uint32_t* b, real* v) {
  const f3 r = unit_vector(a[i], b[i]);
  v[3 * i] = r.x, v[3 * i + 1] = r.y, v[3 * i + 2] = r.z;
}
// the key is one value per call: philox pins it to scalar registers on the device
RT_FN void pb_philox(int i, const uint32_t* ctr, uint32_t k0, uint32_t k1, uint32_t* out) {
  const u4 r = philox(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], k0, k1);
  out[4 * i] = r.x, out[4 * i + 1] = r.y, out[4 * i + 2] = r.z, out[4 * i + 3] = r.w;
}
// acc_add of x into a cleared accumulator (FP32: to_fixed; lo = 0)
RT_FN void pb_acc(int i, const real* x, long long* hi, unsigned long long* lo, int* bad) {
  Acc A;
  acc_clear(A);
  bool b = false;
  acc_add(A, 0, x[i], b);
  hi[i] = A.hi[0];
#if RT_F64
  lo[i] = A.lo[0];
#else
  lo[i] = 0;
#endif
  bad[i] = b ? 1 : 0;
}
// kind: 0 isect_sphere, 1 isect_plane<1>, 2 isect_plane<0>, 3 isect_plane<-1> quad, 4 isect_plane<-1>
// triangle; rec: the 16 reals of a primitive record; tmin_up = float_up(tmin) as prefix_hits forms it.
// take: whether `consider` makes (t, q) the closest hit of a ray that has none yet — the kernel's own
// meaning of "accepted" (a margin q >= 0 with t NaN or +inf is never taken)
RT_FN void pb_isect(int i, int kind, const real* rec, const real* o, const real* d, const real* tmin, const int* self,
                    real* t, real* q, int* take) {
  const real* p = rec + 16 * (size_t)i;
  const PrimRec r{v4{p[0], p[1], p[2], p[3]}, v4{p[4], p[5], p[6], p[7]}, v4{p[8], p[9], p[10], p[11]},
                  v4{p[12], p[13], p[14], p[15]}};
  RayCtx R{};
  R.o = ld3(o + 3 * i);
  R.d = ld3(d + 3 * i);
  const real tm = tmin[i], tu = float_up(tm);
  const bool sf = self[i] != 0;
  real tt = RT_NAN, qq = -RL(1.0);
  switch (kind) {
    case 0: isect_sphere(r, R.o, R, tm, tu, sf, tt, qq); break;
    case 1: isect_plane<1>(r, R.o, R, tu, sf, tt, qq); break;
    case 2: isect_plane<0>(r, R.o, R, tu, sf, tt, qq); break;
    case 3: isect_plane<-1>(r, R.o, R, tu, sf, tt, qq, true); break;
    case 4: isect_plane<-1>(r, R.o, R, tu, sf, tt, qq, false); break;
  }
  t[i] = tt;
  q[i] = qq;
  Closest C = no_hit();
  consider<false>(C, tt, qq, 1, 7);
  take[i] = C.prim == 7 ? 1 : 0;
}
// tg: q, n, wa, wb of a redirect target (12 reals)
RT_FN void pb_target(int i, const real* tg, const real* o, const real* d, int* hit, real* t, real* rinv) {
  RT_NS::DevTarget T{};
  const real* p = tg + 12 * (size_t)i;
  for (int k = 0; k < 3; ++k) T.q[k] = p[k], T.n[k] = p[3 + k], T.wa[k] = p[6 + k], T.wb[k] = p[9 + k];
  real tt = RT_NAN, ri = RT_NAN;
  hit[i] = target_hit(T, ld3(o + 3 * i), ld3(d + 3 * i), tt, ri) ? 1 : 0;
  t[i] = tt;
  rinv[i] = ri;
}
#if RT_NODE_F32
// prep_ray + node_slabs_f32 against one box given as both children: box = (xmin, xmax, ymin, ymax,
// zmin, zmax), tr = (tmin, tmax); accept bit 0 / 1: the left / right child is entered
RT_FN void pb_node(int i, const real* o, const real* d, const float* box, const real* tr, int* accept) {
  RayCtx R{};
  R.o = ld3(o + 3 * i);
  R.d = ld3(d + 3 * i);
  prep_ray(R);
  const float* b = box + 6 * (size_t)i;
  const v4f n0{b[0], b[1], b[2], b[3]}, n1{b[0], b[1], b[2], b[3]}, n2{b[4], b[5], b[4], b[5]};
  float ln, lf, rn, rf;
  node_slabs_f32(R, n0, n1, n2, (float)tr[2 * i], (float)tr[2 * i + 1], ln, lf, rn, rf);
  accept[i] = (ln <= lf ? 1 : 0) | (rn <= rf ? 2 : 0);
}
#endif

// ---- the shading half.  Records the kernel reads through constant-address-space pointers come in
// as arrays of the record's bytes (the host builder's, tests/kernel_emu rt_emu_scene_arrays), and
// the KernelParams member the function reads is pointed at them; only those members are filled.
// eval_texture<true>: element i reads texture record i of `texs` at (u, v) = uv[2 i ..], p = p[3 i ..];
// texels / perm / grad: the tables of the whole call
RT_FN void pb_texture(int i, const unsigned char* texs, const real* texels, const int* perm, const real* grad,
                      const real* uv, const real* p, real* rgb) {
  RT_NS::KernelParams P{};
  P.texs = (const RT_NS::DevTexture*)texs;
  P.texels = texels;
  P.perlin_perm = perm;
  P.perlin_grad = grad;
  const f3 c = eval_texture<true>(P, i, uv[2 * i], uv[2 * i + 1], ld3(p + 3 * i));
  rgb[3 * i] = c.x, rgb[3 * i + 1] = c.y, rgb[3 * i + 2] = c.z;
}
// op 0 perlin_noise(q), otherwise fractal_noise(depth = op, q)
RT_FN void pb_noise(int i, int op, const int* perm, const real* grad, const real* q, real* y) {
  const f3 p = ld3(q + 3 * i);
  y[i] = op == 0 ? perlin_noise((const RT_CAS int*)perm, cf(grad), p)
                 : fractal_noise((const RT_CAS int*)perm, cf(grad), op, p);
}
// surface_info of primitive record i (16 reals) with prim_uv row i (6 reals) for the ray (o, d) at t;
// out: p, n (3 reals each), front, (u, v), gid
RT_FN void pb_surface(int i, int need_uv, const real* prims, const real* prim_uv, const real* uvframes, const real* o,
                      const real* d, const real* t, real* hp, real* hn, int* front, real* uv, int* gid) {
  RT_NS::KernelParams P{};
  P.prims = prims;
  P.prim_uv = prim_uv;
  P.uvframes = uvframes;
  RayCtx R{};
  R.o = ld3(o + 3 * i);
  R.d = ld3(d + 3 * i);
  const HitInfo h = surface_info(P, cf(prims), i, R, t[i], need_uv != 0);
  hp[3 * i] = h.p.x, hp[3 * i + 1] = h.p.y, hp[3 * i + 2] = h.p.z;
  hn[3 * i] = h.n.x, hn[3 * i + 1] = h.n.y, hn[3 * i + 2] = h.n.z;
  front[i] = h.front ? 1 : 0;
  uv[2 * i] = h.u, uv[2 * i + 1] = h.v;
  gid[i] = h.gid;
}
// test_box<false> of box record `box` (one per call: the record is wave-uniform in the kernel) for a
// ray without a hit so far; out: Closest's t (+inf: no hit), primitive and key order (-1: no hit)
RT_FN void pb_box(int i, int box, const unsigned char* boxes, const real* o, const real* d, const real* tmin,
                  const int* self_gid, real* t, int* prim, int* ord) {
  RayCtx R{};
  R.o = ld3(o + 3 * i);
  R.d = ld3(d + 3 * i);
  R.self_gid = self_gid[i];
  R.self_inst = -1;
  Closest C = no_hit();
  test_box<false>((const RT_CAS RT_NS::DevBox*)boxes + box, R, float_up(tmin[i]), C);
  t[i] = C.t;
  prim[i] = C.prim;
#if RT_F64
  ord[i] = C.prim < 0 ? -1 : C.ord;
#else
  ord[i] = C.prim < 0 ? -1 : (int)(unsigned)(C.key & 0xffffffffull);
#endif
}
// medium_draw of medium m[i] (0 .. 3: the word selector) with neg_inv_density nid[i], the Philox block
// w[4 i ..], the segment (lo, hi) = lohi[2 i ..] and the closest hit so far tb[i]
RT_FN void pb_medium(int i, const int* m, const uint32_t* w, const real* nid, const real* lohi, const real* tb,
                     real* tbest, int* hit_medium) {
  RT_NS::KernelParams P{};
  const int mm = m[i] & 3;
  P.media[mm].neg_inv_density = nid[i];
  real t = tb[i];
  int hm = -1;
  medium_draw(P, mm, u4{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]}, lohi[2 * i], lohi[2 * i + 1], t, hm);
  tbest[i] = t;
  hit_medium[i] = hm;
}
// shade_event<2, true, false> (form 1) or <0, false, false> (form 0) of element i.  KP: the call's
// KernelParams BY VALUE, as the render kernels take theirs (philox pins the key to scalar registers, so
// the struct must be a kernel argument, not a per-thread copy); pb_shade_params below fills it on the
// host.  how[i]: 0 a hit on primitive record i (prims, 16 reals) with material record i of KP.prim_shade,
// 1 a medium hit (medium 0, material KP.media[0].material of KP.mats), 2 a miss.  ray: o, d, t (7 reals);
// ctr: pix, sample, seg; LT: L, T (6 reals).  out: terminate, L, np, nd, Tf, ngid (np, nd, Tf, ngid as
// shade() presets them: NaN / RT_EMPTY_ROOT on the emulator; the incoming ray, 1, self_gid = -1 on the device)
RT_FN void pb_shade(int i, int form, const RT_NS::KernelParams& P, const real* prims, const int* how, const real* ray,
                    const uint32_t* ctr, const real* LT, int* term, real* Lo, real* np, real* nd, real* Tf, int* ngid) {
  RayCtx R{};
  R.o = ld3(ray + 7 * i);
  R.d = ld3(ray + 7 * i + 3);
  R.self_gid = -1;
  R.self_inst = -1;
  const real tb = ray[7 * i + 6];
  f3 L = ld3(LT + 6 * i);
  const f3 T = ld3(LT + 6 * i + 3);
#ifdef RT_HOST_EMU
  f3 p2 = mk3(RT_NAN, RT_NAN, RT_NAN), d2 = p2, tf = p2;
  int g2 = RT_EMPTY_ROOT;
#else
  f3 p2 = R.o, d2 = R.d, tf = mk3(RL(1.), RL(1.), RL(1.));
  int g2 = R.self_gid;
#endif
  const int best = how[i] == 0 ? i : -1, hm = how[i] == 1 ? 0 : -1;
  const uint32_t pix = ctr[3 * i];
  const int sample = (int)ctr[3 * i + 1], seg = (int)ctr[3 * i + 2];
  const bool e = form ? shade_event<2, true, false>(P, cf(prims), pix, sample, seg, tb, best, hm, R, L, T, -1, p2, d2, tf, g2)
                      : shade_event<0, false, false>(P, cf(prims), pix, sample, seg, tb, best, hm, R, L, T, -1, p2, d2, tf, g2);
  term[i] = e ? 1 : 0;
  Lo[3 * i] = L.x, Lo[3 * i + 1] = L.y, Lo[3 * i + 2] = L.z;
  np[3 * i] = p2.x, np[3 * i + 1] = p2.y, np[3 * i + 2] = p2.z;
  nd[3 * i] = d2.x, nd[3 * i + 1] = d2.y, nd[3 * i + 2] = d2.z;
  Tf[3 * i] = tf.x, Tf[3 * i + 1] = tf.y, Tf[3 * i + 2] = tf.z;
  ngid[i] = g2;
}
#ifdef RT_HOST_EMU
// The KernelParams of a pb_shade call (host side, both backends): only the members shade_event reads.
// mats: the address (host or device) of the call's DevMaterial records (prim_shade and mats); targets:
// n_targets DevTarget records on the host; cfg: rem_prob, bg_kind, bg0, bg1 (8 doubles).  Returns
// sizeof(KernelParams); the struct is written when cap allows.
static long long pb_shade_params(void* out, long long cap, const void* mats, int med_mat, uint32_t k0, uint32_t k1,
                                 int n_targets, const void* targets, const double* cfg) {
  RT_NS::KernelParams P{};
  if (n_targets < 0 || n_targets > RT_MAX_TARGETS) return -1;
  P.prim_shade = (const RT_NS::DevMaterial*)mats;
  P.mats = (const RT_NS::DevMaterial*)mats;
  P.media[0].material = med_mat;
  P.key0 = k0, P.key1 = k1;
  P.n_targets = n_targets;
  for (int k = 0; k < n_targets; ++k) P.targets[k] = ((const RT_NS::DevTarget*)targets)[k];
  P.rem_prob = (real)cfg[0];
  P.cam.bg_kind = (int)cfg[1];
  for (int k = 0; k < 3; ++k) P.cam.bg0[k] = (real)cfg[2 + k], P.cam.bg1[k] = (real)cfg[5 + k];
  if (out && cap >= (long long)sizeof P) std::memcpy(out, &P, sizeof P);
  return (long long)sizeof P;
}
#endif

#define RT_PROBE_UNPACK(...) __VA_ARGS__
RT_PROBE_DEFINE(math1, (int op, const real* x, real* y), (op, x, y))
RT_PROBE_DEFINE(uniform, (int op, const uint32_t* w, real* y), (op, w, y))
RT_PROBE_DEFINE(sincos, (const uint32_t* w, real* s, real* c), (w, s, c))
RT_PROBE_DEFINE(unit_vector, (const uint32_t* a, const uint32_t* b, real* v), (a, b, v))
RT_PROBE_DEFINE(philox, (const uint32_t* ctr, uint32_t k0, uint32_t k1, uint32_t* out), (ctr, k0, k1, out))
RT_PROBE_DEFINE(acc, (const real* x, long long* hi, unsigned long long* lo, int* bad), (x, hi, lo, bad))
RT_PROBE_DEFINE(isect,
                (int kind, const real* rec, const real* o, const real* d, const real* tmin, const int* self, real* t,
                 real* q, int* take),
                (kind, rec, o, d, tmin, self, t, q, take))
RT_PROBE_DEFINE(target, (const real* tg, const real* o, const real* d, int* hit, real* t, real* rinv),
                (tg, o, d, hit, t, rinv))
RT_PROBE_DEFINE(texture,
                (const unsigned char* texs, const real* texels, const int* perm, const real* grad, const real* uv,
                 const real* p, real* rgb),
                (texs, texels, perm, grad, uv, p, rgb))
RT_PROBE_DEFINE(noise, (int op, const int* perm, const real* grad, const real* q, real* y), (op, perm, grad, q, y))
RT_PROBE_DEFINE(surface,
                (int need_uv, const real* prims, const real* prim_uv, const real* uvframes, const real* o, const real* d,
                 const real* t, real* hp, real* hn, int* front, real* uv, int* gid),
                (need_uv, prims, prim_uv, uvframes, o, d, t, hp, hn, front, uv, gid))
RT_PROBE_DEFINE(box,
                (int box, const unsigned char* boxes, const real* o, const real* d, const real* tmin, const int* self_gid,
                 real* t, int* prim, int* ord),
                (box, boxes, o, d, tmin, self_gid, t, prim, ord))
RT_PROBE_DEFINE(medium,
                (const int* m, const uint32_t* w, const real* nid, const real* lohi, const real* tb, real* tbest,
                 int* hit_medium),
                (m, w, nid, lohi, tb, tbest, hit_medium))
RT_PROBE_DEFINE(shade,
                (int form, RT_NS::KernelParams KP, const real* prims, const int* how, const real* ray,
                 const uint32_t* ctr, const real* LT, int* term, real* Lo, real* np, real* nd, real* Tf, int* ngid),
                (form, KP, prims, how, ray, ctr, LT, term, Lo, np, nd, Tf, ngid))
#if RT_NODE_F32
RT_PROBE_DEFINE(node, (const real* o, const real* d, const float* box, const real* tr, int* accept),
                (o, d, box, tr, accept))
#endif
#undef RT_PROBE_UNPACK
