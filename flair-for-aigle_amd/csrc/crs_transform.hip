// Points from one coordinate reference system to another: one streaming pass over float64 (x, y) pairs, one thread per
// point, a 16-byte load and a 16-byte store each, no LDS, no atomics.  include/flairhip.h holds the normative
// definition (FfaCrs, the datum rule, the NaN rule).
//
// A transform is  source -> geodetic (lon, lat) in radians -> destination; the kernel is instantiated per (source kind,
// destination kind), so a projected -> projected call runs both steps in registers.  Everything that depends on the CRS
// alone is computed once per call on the host (derive) and passed by value.
//
// Datum rule: every supported CRS is on GRS80 or WGS 84 and geodetic longitude / latitude cross between them unchanged
// (the registry's RGF93 -> WGS 84 operation is the null transformation); each projection uses its own ellipsoid.
//
// Both projections are conformal and meet in the isometric latitude
//   psi(lat) = asinh(tan lat) - e atanh(e sin lat),
// whose inverse is the fixed point  s = tanh(psi + e atanh(e s)),  s = sin lat.  The map s -> s contracts by about
// e^2 (1 - s^2) <= 6.7e-3 per round; from s = tanh(psi) (error <= 3.4e-3) eight rounds leave 3.4e-3 * 6.7e-3^8 < 1e-19,
// below the float64 rounding of s: a ninth round changes nothing.  The count is fixed, there is no data-dependent exit.
//
// Lambert conformal conic, two standard parallels (EPSG Guidance Note 7-2, method 9802), with t = exp(-psi):
//   r = a F t^n = a F exp(-n psi),  theta = n (lon - lon0),  E = FE + r sin theta,  N = FN + r0 - r cos theta
//   inverse: r = hypot(E - FE, r0 - (N - FN)) with the sign of n, psi = -log(r / (a F)) / n,
//            lon = lon0 + atan2(E - FE, r0 - (N - FN)) / n  (both arguments negated when n < 0)
// Transverse Mercator (EPSG 9807) by the Krueger series (Karney, "Transverse Mercator with an accuracy of a few
// nanometers", J. Geodesy 85, 2011, eqs. 7-11 and 35-36), through n^6:
//   xi' = atan2(sinh psi, cos dlon),  eta' = atanh(sin dlon / cosh psi),  zeta = xi + i eta
//   zeta = zeta' + sum alpha_j sin(2 j zeta'),  E = FE + k0 A eta,  N = FN + k0 A (xi - xi0)
//   inverse: zeta' = zeta - sum beta_j sin(2 j zeta),  psi = asinh(sin xi' / hypot(sinh eta', cos xi')),
//            dlon = atan2(sinh eta', cos xi')
// FMA contraction is left on: the contract is accuracy, and one code object gives the same bytes for the same input.
#include "ffa_common.h"

#include <cmath>

namespace {

constexpr int kT = 256;
constexpr int kRounds = 8;   // fixed-point rounds of the inverse latitude (see above)
constexpr int kOrder = 6;    // Krueger series: terms through n^6
constexpr double kDeg = 0.017453292519943295769;  // pi / 180
constexpr double kRad = 57.295779513082320877;    // 180 / pi

// what the kernel needs of one CRS: derived on the host, passed by value
struct Proj {
  double e;             // first eccentricity
  double lon0;          // radians
  double fe, fn;
  double scale;         // conic: a F;  transverse Mercator: k0 A
  double n;             // conic: cone constant
  double r0;            // conic: radius of the latitude of origin
  double xi0;           // transverse Mercator: rectifying latitude of the latitude of origin
  double alpha[kOrder]; // forward series
  double beta[kOrder];  // inverse series
};

__host__ __device__ inline double iso_lat(double lat, double e) {
  return asinh(tan(lat)) - e * atanh(e * sin(lat));
}

__host__ __device__ inline double lat_from_iso(double psi, double e) {
  double s = tanh(psi);
#pragma unroll
  for (int k = 0; k < kRounds; ++k) s = tanh(psi + e * atanh(e * s));
  return atan(sinh(psi + e * atanh(e * s)));
}

// zeta + sign * sum c_j sin(2 j zeta) for zeta = xi + i eta; sin / cos of the multiples by the addition theorem
__host__ __device__ inline void krueger(const double* c, double sign, double& xi, double& eta) {
  const double s2 = sin(2.0 * xi), c2 = cos(2.0 * xi), sh = sinh(2.0 * eta), ch = cosh(2.0 * eta);
  const double s1r = s2 * ch, s1i = c2 * sh;   // sin(2 zeta)
  const double c1r = c2 * ch, c1i = -s2 * sh;  // cos(2 zeta)
  double sr = s1r, si = s1i, cr = c1r, ci = c1i;
  double ar = 0.0, ai = 0.0;
#pragma unroll
  for (int j = 0; j < kOrder; ++j) {
    ar += c[j] * sr;
    ai += c[j] * si;
    // sin(2 (j + 1) zeta) = s_j c_1 + c_j s_1,  cos(2 (j + 1) zeta) = c_j c_1 - s_j s_1  (complex products)
    const double nsr = (sr * c1r - si * c1i) + (cr * s1r - ci * s1i);
    const double nsi = (sr * c1i + si * c1r) + (cr * s1i + ci * s1r);
    const double ncr = (cr * c1r - ci * c1i) - (sr * s1r - si * s1i);
    const double nci = (cr * c1i + ci * c1r) - (sr * s1i + si * s1r);
    sr = nsr; si = nsi; cr = ncr; ci = nci;
  }
  xi += sign * ar;
  eta += sign * ai;
}

// ---- source CRS -> geodetic radians; false when the point has no image ---------------------------------------------

template <int KIND>
__host__ __device__ inline bool to_geodetic(const Proj& p, double x, double y, double& lon, double& lat) {
  if (KIND == FFA_CRS_GEOGRAPHIC) {
    lon = x * kDeg;
    lat = y * kDeg;
    return fabs(y) <= 90.0;
  } else if (KIND == FFA_CRS_LCC2SP) {
    double dx = x - p.fe, dy = p.r0 - (y - p.fn);
    double r = hypot(dx, dy);
    if (!(r > 0.0)) return false;  // the pole of the cone (and NaN)
    if (p.n < 0.0) { dx = -dx; dy = -dy; }
    const double psi = -log(r / fabs(p.scale)) / p.n;
    lon = p.lon0 + atan2(dx, dy) / p.n;
    lat = lat_from_iso(psi, p.e);
    return true;
  } else {
    double xi = (y - p.fn) / p.scale + p.xi0, eta = (x - p.fe) / p.scale;
    krueger(p.beta, -1.0, xi, eta);
    const double sh = sinh(eta), c = cos(xi);
    const double psi = asinh(sin(xi) / hypot(sh, c));
    lon = p.lon0 + atan2(sh, c);
    lat = lat_from_iso(psi, p.e);
    return true;
  }
}

// ---- geodetic radians -> destination CRS ---------------------------------------------------------------------------

template <int KIND>
__host__ __device__ inline void from_geodetic(const Proj& p, double lon, double lat, double& x, double& y) {
  if (KIND == FFA_CRS_GEOGRAPHIC) {
    x = lon * kRad;
    y = lat * kRad;
  } else if (KIND == FFA_CRS_LCC2SP) {
    const double r = p.scale * exp(-p.n * iso_lat(lat, p.e));
    const double theta = p.n * (lon - p.lon0);
    x = p.fe + r * sin(theta);
    y = p.fn + p.r0 - r * cos(theta);
  } else {
    const double psi = iso_lat(lat, p.e), dlon = lon - p.lon0;
    const double sp = sinh(psi), cl = cos(dlon);
    double xi = atan2(sp, cl), eta = asinh(sin(dlon) / hypot(sp, cl));
    krueger(p.alpha, 1.0, xi, eta);
    x = p.fe + p.scale * eta;
    y = p.fn + p.scale * (xi - p.xi0);
  }
}

template <int SK, int DK>
__global__ __launch_bounds__(kT) void crs_transform_kernel(const double2* in, double2* out, long long n, Proj src,
                                                           Proj dst) {
  const long long i = (long long)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const double2 p = in[i];  // in may be out: this thread's own element, read before it is written
  double lon, lat, x = 0.0, y = 0.0;
  bool ok = isfinite(p.x) && isfinite(p.y) && to_geodetic<SK>(src, p.x, p.y, lon, lat);
  if (ok) {
    from_geodetic<DK>(dst, lon, lat, x, y);
    ok = isfinite(x) && isfinite(y);
  }
  const double nan = __builtin_nan("");
  out[i] = ok ? make_double2(x, y) : make_double2(nan, nan);
}

// ---- host: constants of one CRS ------------------------------------------------------------------------------------

bool derive(const FfaCrs& c, const char* which, Proj* out) {
  Proj p = {};
  if (c.kind == FFA_CRS_GEOGRAPHIC) {
    *out = p;
    return true;
  }
  if (c.kind != FFA_CRS_LCC2SP && c.kind != FFA_CRS_TMERC) {
    ffa_set_error("crs_transform: %s kind %d is none of geographic, lcc2sp, tmerc", which, c.kind);
    return false;
  }
  if (!(c.a > 0.0) || !(c.inv_flattening > 1.0) || !std::isfinite(c.a) || !std::isfinite(c.inv_flattening) ||
      !std::isfinite(c.lon0) || !(std::fabs(c.lat0) <= 90.0) || !std::isfinite(c.false_easting) ||
      !std::isfinite(c.false_northing)) {
    ffa_set_error("crs_transform: %s ellipsoid (a %g, 1/f %g), origin (%g, %g) or false origin not usable", which, c.a,
                  c.inv_flattening, c.lon0, c.lat0);
    return false;
  }
  const double f = 1.0 / c.inv_flattening;
  p.e = std::sqrt(f * (2.0 - f));
  p.lon0 = c.lon0 * kDeg;
  p.fe = c.false_easting;
  p.fn = c.false_northing;
  if (c.kind == FFA_CRS_LCC2SP) {
    if (!(std::fabs(c.lat1) < 90.0) || !(std::fabs(c.lat2) < 90.0) || !(std::fabs(c.lat0) < 90.0) ||
        c.lat1 + c.lat2 == 0.0) {
      ffa_set_error("crs_transform: %s standard parallels %g, %g (origin %g) do not define a cone", which, c.lat1,
                    c.lat2, c.lat0);
      return false;
    }
    const double e2 = p.e * p.e;
    auto m = [&](double lat) { return std::cos(lat) / std::sqrt(1.0 - e2 * std::sin(lat) * std::sin(lat)); };
    const double l1 = c.lat1 * kDeg, l2 = c.lat2 * kDeg;
    const double psi1 = iso_lat(l1, p.e), psi2 = iso_lat(l2, p.e);  // ln t = -psi
    // one standard parallel given twice: the cone constant is its sine (the limit of the quotient)
    p.n = c.lat1 == c.lat2 ? std::sin(l1) : (std::log(m(l1)) - std::log(m(l2))) / (psi2 - psi1);
    const double F = m(l1) * std::exp(p.n * psi1) / p.n;
    p.scale = c.a * F;
    p.r0 = p.scale * std::exp(-p.n * iso_lat(c.lat0 * kDeg, p.e));
  } else {
    if (!(c.k0 > 0.0) || !std::isfinite(c.k0)) {
      ffa_set_error("crs_transform: %s scale factor %g", which, c.k0);
      return false;
    }
    const double n = f / (2.0 - f), n2 = n * n, n3 = n2 * n, n4 = n3 * n, n5 = n4 * n, n6 = n5 * n;
    const double A = c.a / (1.0 + n) * (1.0 + n2 / 4.0 + n4 / 64.0 + n6 / 256.0);
    p.scale = c.k0 * A;
    // Karney 2011, eq. 35 (alpha) and eq. 36 (beta)
    p.alpha[0] = n / 2 - 2 * n2 / 3 + 5 * n3 / 16 + 41 * n4 / 180 - 127 * n5 / 288 + 7891 * n6 / 37800;
    p.alpha[1] = 13 * n2 / 48 - 3 * n3 / 5 + 557 * n4 / 1440 + 281 * n5 / 630 - 1983433 * n6 / 1935360;
    p.alpha[2] = 61 * n3 / 240 - 103 * n4 / 140 + 15061 * n5 / 26880 + 167603 * n6 / 181440;
    p.alpha[3] = 49561 * n4 / 161280 - 179 * n5 / 168 + 6601661 * n6 / 7257600;
    p.alpha[4] = 34729 * n5 / 80640 - 3418889 * n6 / 1995840;
    p.alpha[5] = 212378941 * n6 / 319334400;
    p.beta[0] = n / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800;
    p.beta[1] = n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720;
    p.beta[2] = 17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720;
    p.beta[3] = 4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600;
    p.beta[4] = 4583 * n5 / 161280 - 108847 * n6 / 3991680;
    p.beta[5] = 20648693 * n6 / 638668800;
    // rectifying latitude of the origin: the forward series on the central meridian
    double xi = std::atan(std::sinh(iso_lat(c.lat0 * kDeg, p.e))), eta = 0.0;
    krueger(p.alpha, 1.0, xi, eta);
    p.xi0 = xi;
  }
  if (!std::isfinite(p.scale) || p.scale == 0.0 || !std::isfinite(p.r0) || !std::isfinite(p.n)) {
    ffa_set_error("crs_transform: %s parameters give no finite projection constants", which);
    return false;
  }
  *out = p;
  return true;
}

template <int SK, int DK>
void launch(const double* in, double* out, long long n, const Proj& s, const Proj& d, hipStream_t st) {
  const unsigned int blocks = (unsigned int)((n + kT - 1) / kT);
  hipLaunchKernelGGL((crs_transform_kernel<SK, DK>), dim3(blocks), dim3(kT), 0, st,
                     reinterpret_cast<const double2*>(in), reinterpret_cast<double2*>(out), n, s, d);
}

template <int SK>
void launch_dst(int dk, const double* in, double* out, long long n, const Proj& s, const Proj& d, hipStream_t st) {
  if (dk == FFA_CRS_GEOGRAPHIC) launch<SK, FFA_CRS_GEOGRAPHIC>(in, out, n, s, d, st);
  else if (dk == FFA_CRS_LCC2SP) launch<SK, FFA_CRS_LCC2SP>(in, out, n, s, d, st);
  else launch<SK, FFA_CRS_TMERC>(in, out, n, s, d, st);
}

}  // namespace

extern "C" int ffa_crs_transform_f64(const double* in, double* out, long long n, const FfaCrs* src, const FfaCrs* dst,
                                     hipStream_t st) {
  FFA_REQUIRE(src && dst, "crs_transform: null CRS");
  FFA_REQUIRE(n >= 0 && n <= 0xffffff00ll, "crs_transform: %lld points outside 0 .. 2^32 - 256", n);
  Proj s, d;
  if (!derive(*src, "source", &s) || !derive(*dst, "destination", &d)) return FFA_ERR_ARG;
  if (n == 0) return FFA_OK;
  FFA_REQUIRE(in && out, "crs_transform: null pointer");
  FFA_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0,
              "crs_transform: points must be 16-byte aligned (in %p, out %p)", (const void*)in, (void*)out);
  if (src->kind == FFA_CRS_GEOGRAPHIC) launch_dst<FFA_CRS_GEOGRAPHIC>(dst->kind, in, out, n, s, d, st);
  else if (src->kind == FFA_CRS_LCC2SP) launch_dst<FFA_CRS_LCC2SP>(dst->kind, in, out, n, s, d, st);
  else launch_dst<FFA_CRS_TMERC>(dst->kind, in, out, n, s, d, st);
  return ffa_check_launch("crs_transform");
}
