// gc_binsdev.h — device primitives of the bins kernels (gc_bins.hip, gc_moments.hip, gc_binstask.h): the
// 16-lane DPP sums, the Newton reciprocals, the 2048-entry table exp, the bins epilogue's log, the series
// deskew and the per-point direction / window / feature helpers. No kernel and no device variable lives
// here: the exp table itself belongs to gc_bins.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gc_math.h"

namespace gc {

typedef double v4d __attribute__((ext_vector_type(4)));  // f64 MFMA accumulator (4 per lane)

// 16-lane (DPP row) butterflies: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror,
// row_mirror. Every step pairs each lane with a distinct partner holding a disjoint partial, so
// all 16 lanes end with the bit-identical total; no LDS round trip (ds_bpermute) on the path.
template <int CTRL>
GC_DEV double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;

GC_DEV double group16_sum(double v) {
  v += dpp_f64<kDppXor1>(v);
  v += dpp_f64<kDppXor2>(v);
  v += dpp_f64<kDppHalfMirror>(v);
  v += dpp_f64<kDppMirror>(v);
  return v;
}

constexpr double kRoundMagic = 6755399441055744.0;  // 1.5 * 2^52: fma(y, c, M) - M = rint(y c)
// 1/z for z > 0 in a normal range, one Newton step on the hardware reciprocal (a few ulp; the
// fused kernel's softmax normaliser, where it is one of ~140 issue slots per step)
GC_DEV double recip1(double z) {
  const double r = __builtin_amdgcn_rcp(z);
  return fma(r, fma(-z, r, 1.0), r);
}
// 1/z for z > 0 in a normal range: hardware reciprocal + two Newton steps (<= 1 ulp).
GC_DEV double recip(double z) {
  double r = __builtin_amdgcn_rcp(z);
  double e = fma(-z, r, 1.0);
  r = fma(r, e, r);
  e = fma(-z, r, 1.0);
  return fma(r, e, r);
}
// The 16-lane sums of two steps at once, as a reduce-scatter: the butterfly above leaves one number in
// all 16 lanes of a row and every lane then takes the same reciprocal; here the first exchange round
// halves the values a lane carries, so two steps' sums cost 4 adds and 1 reciprocal instead of 8 and 2.
//   round 1 (lane bit 0): a lane keeps the step of its own parity of the pair (z0, z1) and sends the other
//     to its xor-1 partner: even lanes hold the pair sums of step 0, odd lanes those of step 1;
//   round 2: the butterfly's xor 2, which keeps the parity of the lane;
//   rounds 3, 4: row_shl:4 then row_shl:8 (lane l reads lane l + 4, l + 8 of its row; a source past the
//     row reads 0): lanes of one parity only ever meet their own parity, so lanes 0 and 1 of each row end
//     with the totals of steps 0 and 1 (the row mirrors of group16_sum reverse a quad and would mix the
//     steps). The other lanes hold partial sums nobody reads.
// Per step the additions are those of the butterfly in its association, ((l0 + l1) + (l2 + l3)) per
// quad, then (Q0 + Q1) + (Q2 + Q3), with operands swapped at most: the same bits. One recip1 on the
// lane's own total, then Z and 1/Z of step s go back to the row's 16 lanes by row_newbcast:s, a 64-bit
// DPP move each (the only DPP control the f64 pipe of gfx90a and later takes on a 64-bit operand).
// H = 256 1.1529 -> 1.1336 ms per step against the per-step butterfly, H = 32 no slower; a batch of four
// steps measured 1.1351 and spilled more (profiles/r07/ab_bins_zbatch.txt). The butterfly's exchanges as
// ds_swizzle on the LDS pipe measured 15 % slower (profiles/r06/ab_zsum_swizzle.txt).
constexpr int kDppRowShl4 = 0x104, kDppRowShl8 = 0x108, kDppRowBcast0 = 0x150;
template <int CTRL>
GC_DEV double dpp_f64_z(double v) {  // dpp_f64 with 0 for a source lane outside the row
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
template <int LANE>
GC_DEV double row_bcast_f64(double v) {  // lane LANE of the row to its 16 lanes: one v_mov_b64_dpp
  return __builtin_amdgcn_update_dpp(0.0, v, kDppRowBcast0 + LANE, 0xF, 0xF, true);
}
GC_DEV void group16_sum2(const double (&z)[2], int lane, double (&Z)[2], double (&rZ)[2]) {
  const bool b0 = (lane & 1) != 0;
  double q = (b0 ? z[1] : z[0]) + dpp_f64<kDppXor1>(b0 ? z[0] : z[1]);
  q += dpp_f64<kDppXor2>(q);
  q += dpp_f64_z<kDppRowShl4>(q);
  q += dpp_f64_z<kDppRowShl8>(q);
  const double rq = recip1(q);
  Z[0] = row_bcast_f64<0>(q); rZ[0] = row_bcast_f64<0>(rq);
  Z[1] = row_bcast_f64<1>(q); rZ[1] = row_bcast_f64<1>(rq);
}
// A double whose bits the compiler cannot see: two v_mov_b32 at the point of use. In a persistent
// kernel at 256 VGPRs a plain 64-bit constant is hoisted out of the task loop and spilled, and a
// polynomial then reloads each coefficient from scratch in a serial chain (the epilogue's log:
// six dependent scratch round trips per task)
template <int HI, int LO>
GC_DEV double vconst() {
  int h, l;
  asm volatile("v_mov_b32 %0, %1" : "=v"(l) : "i"(LO));
  asm volatile("v_mov_b32 %0, %1" : "=v"(h) : "i"(HI));
  return __hiloint2double(h, l);
}
// ln x for a positive normal x (the bins epilogue's log of Π Z): x = 2^k m with m in [√½, √2),
// f = m − 1, s = f/(2 + f), ln m = f − (f²/2 − s(f²/2 + R(s²))) with R the degree-7 minimax
// polynomial in s² of the classic fdlibm __ieee754_log; < 1 ulp there, within 2 ulp with the
// Newton reciprocal for 1/(2 + f). Every coefficient is a vconst.
GC_DEV double log_pos(double x) {
  int k;
  double m = frexp(x, &k);
  if (m < 0.70710678118654752440) {
    m *= 2.0;
    --k;
  }
  const double f = m - 1.0;
  const double s = f * recip(2.0 + f);
  const double z = s * s, w = z * z;
  const double t1 = w * (vconst<0x3FD99999, (int)0x9997FA04>() +
                         w * (vconst<0x3FCC71C5, 0x1D8E78AF>() + w * vconst<0x3FC39A09, (int)0xD078C69F>()));
  const double t2 = z * (vconst<0x3FE55555, 0x55555593>() +
                         w * (vconst<0x3FD24924, (int)0x94229359>() +
                              w * (vconst<0x3FC74664, (int)0x96CB03DE>() + w * vconst<0x3FC2F112, (int)0xDF3E5244>())));
  const double R = t2 + t1, hfsq = 0.5 * f * f, dk = (double)k;
  return dk * vconst<0x3FE62E42, (int)0xFEE00000>() -
         ((hfsq - (s * (hfsq + R) + dk * vconst<0x3DEA39EF, 0x35793C76>())) - f);
}
// the per-point entropy shift of the bins epilogue, (ymax ln2/2048 − B ε)/4 with ymax = ceil(2048/(τ ln2)),
// re-formed from the launch scalars each task (a loop-invariant double here is hoisted and spilled)
GC_DEV double ent_shift(double inv_tau, int B) {
  asm volatile("" : "+v"(inv_tau), "+v"(B));
  const double ymax = ceil(inv_tau * vconst<0x40A71547, 0x652B82FE>());  // 2048 / ln2
  return (ymax * vconst<0x3F362E42, (int)0xFEFA932F>() - (double)B * 1e-12) * 0.25;  // ln2 / 2048
}
// Fused-kernel exp: a 2048-entry table and arguments pre-scaled to y = x·2048/ln2. Entry j holds
// 2^(j/2048) with (j << 9) subtracted from its high word, so adding (k << 9) to the high word of
// T[k & 2047] yields 2^(j/2048)·2^(k >> 11) for any k (one integer add instead of a shift and a
// v_ldexp). r = y - rint(y) is exact (Sterbenz), |r| <= 1/2, and e^{r ln2/2048} needs only a
// cubic (truncation (ln2/4096)^4/24 = 3.5e-17). 13 VALU slots per exp with the 3-FMA logit.
// Valid for y in [-2048·700/ln2, 0] (normal results).
constexpr int kExpTab2 = 2048;
constexpr double kTab2OverLn2 = 2954.6394437405970;     // 2048 / ln2
constexpr double kExp2C1 = 3.3845077175902435e-04;     // ln2 / 2048
constexpr double kExp2C2 = kExp2C1 * kExp2C1 * 0.5;
constexpr double kExp2C3 = kExp2C1 * kExp2C1 * kExp2C1 * (1.0 / 6.0);
GC_DEV void exp_table2_init(double* T) {
  for (int j = threadIdx.x; j < kExpTab2; j += blockDim.x) {
    const double v = exp2((double)j / kExpTab2);
    T[j] = __hiloint2double(__double2hiint(v) - (j << 9), __double2loint(v));
  }
}
template <int N>
GC_DEV void exp2s_n(const double (&y)[N], const double* T, double (&out)[N]) {
  double r[N], tv[N];
  int ki[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double ks = y[j] + kRoundMagic;
    ki[j] = __double2loint(ks);
    r[j] = y[j] - (ks - kRoundMagic);
    tv[j] = T[ki[j] & (kExpTab2 - 1)];
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double p = fma(fma(fma(kExp2C3, r[j], kExp2C2), r[j], kExp2C1), r[j], 1.0);
    const double t = __hiloint2double(__double2hiint(tv[j]) + (ki[j] << 9), __double2loint(tv[j]));
    out[j] = t * p;
  }
}
// exp2s_n of y - m for an integer-valued shift m (Mp = kRoundMagic - m): ks = y + Mp rounds to
// Mp + rint(y), so r = y - (ks - Mp) = y - rint(y) exactly and lo(ks) = rint(y) - m. The shift rides
// in the rounding constant, so the fused logit needs no "- ymax" term of its own.
template <int N>
GC_DEV void exp2s_shift_n(const double (&y)[N], double Mp, const double* T, double (&out)[N]) {
  double r[N], tv[N];
  int ki[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double ks = y[j] + Mp;
    ki[j] = __double2loint(ks);
    r[j] = y[j] - (ks - Mp);
    tv[j] = T[ki[j] & (kExpTab2 - 1)];
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double p = fma(fma(fma(kExp2C3, r[j], kExp2C2), r[j], kExp2C1), r[j], 1.0);
    const double t = __hiloint2double(__double2hiint(tv[j]) + (ki[j] << 9), __double2loint(tv[j]));
    out[j] = t * p;
  }
}
// exp2s_shift_n reading the table at a fixed LDS byte address TAB. The kernels calling this have no
// static LDS (their dynamic block starts at address 0; the launchers check it, ensure_no_static_lds), so
// the table base folds into the ds_read's immediate offset: the entry's address is (k & 2047) << 3
// with no add of a relocated base per exp. Same values as exp2s_shift_n.
typedef const __attribute__((address_space(3))) char* lds_cptr;
template <int N, unsigned TAB>
GC_DEV void exp2s_shift_tab_n(const double (&y)[N], double Mp, double (&out)[N]) {
  double r[N], tv[N];
  int ki[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double ks = y[j] + Mp;
    ki[j] = __double2loint(ks);
    r[j] = y[j] - (ks - Mp);
    tv[j] = *reinterpret_cast<const __attribute__((address_space(3))) double*>(
        reinterpret_cast<lds_cptr>((uintptr_t)TAB) + ((unsigned)(ki[j] & (kExpTab2 - 1)) << 3));
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double p = fma(fma(fma(kExp2C3, r[j], kExp2C2), r[j], kExp2C1), r[j], 1.0);
    const double t = __hiloint2double(__double2hiint(tv[j]) + (ki[j] << 9), __double2loint(tv[j]));
    out[j] = t * p;
  }
}
// exp2s_shift_tab_n left as its two factors, out[j] = t[j] * p[j] (table entry with the exponent spliced
// in, cubic): for a caller that fuses the product into a sum.
template <int N, unsigned TAB>
GC_DEV void exp2s_shift_tab_tp_n(const double (&y)[N], double Mp, double (&t)[N], double (&p)[N]) {
  double r[N], tv[N];
  int ki[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double ks = y[j] + Mp;
    ki[j] = __double2loint(ks);
    r[j] = y[j] - (ks - Mp);
    tv[j] = *reinterpret_cast<const __attribute__((address_space(3))) double*>(
        reinterpret_cast<lds_cptr>((uintptr_t)TAB) + ((unsigned)(ki[j] & (kExpTab2 - 1)) << 3));
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    p[j] = fma(fma(fma(kExp2C3, r[j], kExp2C2), r[j], kExp2C1), r[j], 1.0);
    t[j] = __hiloint2double(__double2hiint(tv[j]) + (ki[j] << 9), __double2loint(tv[j]));
  }
}
// σ(x) = 1 / (1 + e^{-x}) on the 2048 table (e^{-|x|} clamped at e^{-700} ~ 1e-304)
GC_DEV double sigmoid2(double x, const double* T) {
  const double y[1] = {fmax(-fabs(x), -700.0) * kTab2OverLn2};
  double e[1];
  exp2s_n<1>(y, T, e);
  const double r = recip(1.0 + e[0]);
  return x >= 0.0 ? r : e[0] * r;
}

GC_DEV void lds_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Fused-kernel variants of the three per-point helpers: reciprocals (hardware rcp + 2 Newton
// steps, <= 1 ulp) instead of IEEE divisions and the LDS-table exp in the window sigmoid.
// Results agree with the exact forms to a few ulps; they feed only floating-point moments
// (the bit-exact bin-index contract runs through direction() / k_point_dirs).
GC_DEV void deskew_point_fast(const double* p, double alpha, const double* xi, double* out) {
  const double rho[3] = {alpha * xi[0], alpha * xi[1], alpha * xi[2]};
  const double phi[3] = {alpha * xi[3], alpha * xi[4], alpha * xi[5]};
  const double ts = dot3(phi, phi);
  const double th = sqrt(ts);
  double Bv, Cv, a, b;
  if (th < kSmallAngle) {
    Bv = 0.5 - ts * (1.0 / 24.0);
    Cv = 1.0 / 6.0 - ts * (1.0 / 120.0);
    a = 1.0;
    b = 0.5;
  } else {
    double sn, c;
    sincos(th, &sn, &c);
    const double its = recip((ts < kSmallAngle * kSmallAngle) ? 1.0 : ts);
    const double ith = recip(th);
    Bv = (1.0 - c) * its;
    Cv = (th - sn) * its * ith;
    a = sn * ith;
    b = Bv;
  }
  double V[9], R[9], t[3], q[3];
  rodrigues_form(phi, Bv, Cv, V);
  mat3_vec(V, rho, t);
  rodrigues_form(phi, a, b, R);
  q[0] = p[0] - t[0]; q[1] = p[1] - t[1]; q[2] = p[2] - t[2];
  mat3_tvec(R, q, out);
}
// Series form for the fused kernel: a = sin θ/θ, B = (1 - cos θ)/θ², C = (θ - sin θ)/θ³ are
// power series in θ² (1/(2k+1)!, 1/(2k+2)!, 1/(2k+3)! of (-θ²)^k); ten terms reach < 1e-17 for
// θ² <= 1 — three independent Horner chains instead of sqrt + sincos + two reciprocals. Larger
// rotations (|α ω| > 1 rad within one scan) take the sincos form.
constexpr double kInvFact[22] = {1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889, 0.0001984126984126984, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08, 2.08767569878681e-09, 1.6059043836821613e-10, 1.1470745597729725e-11, 7.647163731819816e-13, 4.779477332387385e-14, 2.8114572543455206e-15, 1.5619206968586225e-16, 8.22063524662433e-18, 4.110317623312165e-19, 1.9572941063391263e-20};
// Fused-kernel deskew in cross-product form: V ρ = ρ + B φ×ρ + C φ×(φ×ρ) and Rᵀ q = q − a φ×q + B φ×(φ×q)
// (the same Rodrigues matrices applied as vectors: 4 cross products instead of two 3x3 forms and two
// matrix-vector products). SHORT: the series for θ² <= kDeskewShortTs (six terms, first omitted term
// < 1e-18 relative), chosen wave-uniformly by the caller; otherwise ten terms (θ² <= 1), and the
// sincos form beyond.
constexpr double kDeskewShortTs = 0.04;
template <bool SHORT>
GC_DEV void deskew_point_cross(const double* p, double alpha, const double* xi, double* out) {
  const double phi[3] = {alpha * xi[3], alpha * xi[4], alpha * xi[5]};
  const double ts = dot3(phi, phi);
  if (!SHORT && ts > 1.0) {
    deskew_point_fast(p, alpha, xi, out);
    return;
  }
  const double rho[3] = {alpha * xi[0], alpha * xi[1], alpha * xi[2]};
  const double u = -ts;
  constexpr int K = SHORT ? 5 : 9;  // highest power of θ² kept
  double a = kInvFact[2 * K + 1], Bv = kInvFact[2 * K + 2], Cv = kInvFact[2 * K + 3];
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    a = fma(a, u, kInvFact[2 * k + 1]);
    Bv = fma(Bv, u, kInvFact[2 * k + 2]);
    Cv = fma(Cv, u, kInvFact[2 * k + 3]);
  }
  double c1[3], c2[3], q[3];
  cross3(phi, rho, c1);
  cross3(phi, c1, c2);
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = p[k] - fma(Cv, c2[k], fma(Bv, c1[k], rho[k]));
  cross3(phi, q, c1);
  cross3(phi, c1, c2);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = fma(Bv, c2[k], fma(-a, c1[k], q[k]));
}
// point_features with w folded into the first factor of each product (w d_i d_j as (w d_i) d_j)
GC_DEV void point_features_w(const double* p, const double* d, double w, double* f) {
  const double wd[3] = {w * d[0], w * d[1], w * d[2]};
  const double wp[3] = {w * p[0], w * p[1], w * p[2]};
  f[0] = w;
  f[1] = wd[0]; f[2] = wd[1]; f[3] = wd[2];
  f[4] = wd[0] * d[0]; f[5] = wd[0] * d[1]; f[6] = wd[0] * d[2];
  f[7] = wd[1] * d[1]; f[8] = wd[1] * d[2]; f[9] = wd[2] * d[2];
  f[10] = wp[0]; f[11] = wp[1]; f[12] = wp[2];
  f[13] = wp[0] * p[0]; f[14] = wp[0] * p[1]; f[15] = wp[0] * p[2];
  f[16] = wp[1] * p[1]; f[17] = wp[1] * p[2]; f[18] = wp[2] * p[2];
}
GC_DEV void direction_fast(const double* p, const double* o, double eps, double* d) {
  const double r0 = p[0] - o[0], r1 = p[1] - o[1], r2 = p[2] - o[2];
  const double inv = recip(sqrt(r0 * r0 + r1 * r1 + r2 * r2) + eps);
  d[0] = r0 * inv; d[1] = r1 * inv; d[2] = r2 * inv;
}
GC_DEV double window_weight2(double t, double t0, double t1, double inv_sig, const double* T) {
  const double wr = sigmoid2((t - t0) * inv_sig, T) * sigmoid2((t1 - t) * inv_sig, T);
  return wr * (1.0 - 1e-12) + 1e-12;
}

// Features g (pre-multiplied by w) for the moment sums of binning.py:160-173.
GC_DEV void point_features(const double* p, const double* d, double w, double* f) {
  f[0] = w;
  f[1] = w * d[0]; f[2] = w * d[1]; f[3] = w * d[2];
  f[4] = w * (d[0] * d[0]); f[5] = w * (d[0] * d[1]); f[6] = w * (d[0] * d[2]);
  f[7] = w * (d[1] * d[1]); f[8] = w * (d[1] * d[2]); f[9] = w * (d[2] * d[2]);
  f[10] = w * p[0]; f[11] = w * p[1]; f[12] = w * p[2];
  f[13] = w * (p[0] * p[0]); f[14] = w * (p[0] * p[1]); f[15] = w * (p[0] * p[2]);
  f[16] = w * (p[1] * p[1]); f[17] = w * (p[1] * p[2]); f[18] = w * (p[2] * p[2]);
}

}  // namespace gc
