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
#if RT_NODE_F32
RT_PROBE_DEFINE(node, (const real* o, const real* d, const float* box, const real* tr, int* accept),
                (o, d, box, tr, accept))
#endif
#undef RT_PROBE_UNPACK
