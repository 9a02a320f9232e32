// Solar elevation of an element: the element part of physics_methods.solar_elevation.
//
//   solar_declination   models/physics_methods.py:997-1010     host, once per call (Python's and NumPy's own arithmetic)
//   equation_of_time    models/physics_methods.py:1013-1023    host, once per call
//   hour_angle          models/physics_methods.py:1026-1033    solar_hour_angle
//   solar_elevation     models/physics_methods.py:1036-1043    solar_elevation_deg
//
// What depends on the time only -- the declination d_rad = deg2rad(solar_declination(time)), the equation of time [minutes] and
// the minutes of the day -- are float64 scalars of the caller; sin(d_rad) and cos(d_rad) are formed once on the host.  The
// element part is float64 in the reference's operation order, one IEEE double operation each, without contraction:
//   time_offset = eqtime + 4 * longitude;  true_solar_time = day_minutes + time_offset;  h = true_solar_time / 4.0 - 180.0
//   elevation = rad2deg(arcsin(sin(deg2rad(lat)) * sin(d_rad) + cos(deg2rad(lat)) * cos(d_rad) * cos(deg2rad(h))))
// with deg2rad(x) = x * (pi / 180) and rad2deg(x) = x * (180 / pi), NumPy's.  sin, cos and asin are the device library's (the
// host's libm in the host build): neither they nor NumPy's are correctly rounded, so the elevation is NOT bit for bit the
// reference's; DESIGN.md section 7h has the measured distance.  longitude and latitude are the float64 the particle set holds
// (LarvalFishExtended._apply_vertical_behavior casts its float32 element arrays to float64 before the call).
//
// Compiled for the CPU by tests/larvalx_host.cpp: includes nothing.
#pragma once

namespace odr {

#define ODR_DEG2RAD (3.141592653589793238462643383279502884 / 180.0)
#define ODR_RAD2DEG (180.0 / 3.141592653589793238462643383279502884)

// hour_angle (:1026-1033) [deg]
__host__ __device__ __forceinline__ double solar_hour_angle(double lon, double eqtime_minutes, double day_minutes) {
  const double time_offset = __dadd_rn(eqtime_minutes, __dmul_rn(4.0, lon));
  const double true_solar_time = __dadd_rn(day_minutes, time_offset);
  return __dsub_rn(__ddiv_rn(true_solar_time, 4.0), 180.0);
}

// solar_elevation (:1036-1043) [deg]; sin_d, cos_d: of the declination in radians
__host__ __device__ __forceinline__ double solar_elevation_deg(double lon, double lat, double sin_d, double cos_d, double eqtime_minutes,
                                                               double day_minutes) {
  const double h = __dmul_rn(solar_hour_angle(lon, eqtime_minutes, day_minutes), ODR_DEG2RAD);
  const double phi = __dmul_rn(lat, ODR_DEG2RAD);
  const double s = __dadd_rn(__dmul_rn(sin(phi), sin_d), __dmul_rn(__dmul_rn(cos(phi), cos_d), cos(h)));
  return __dmul_rn(asin(s), ODR_RAD2DEG);
}

}  // namespace odr
