// libodrift_hip.so, a translation unit of its own: the ship model's own physics (ShipDrift.update: wind force, wave-drift force
// from the spectrum, wave damping and form drag, the two moves, stranding).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_ship.hip.h"

// The class tables of a run on the device: n_classes x 49 x 2 doubles (F, D at the 49 spectrum points below omega = 7), kept with
// their count.
struct odr_ship_table {
  double *dev;
  int n_classes;
};

int odr_ship_table_create(odr_ctx *c, const double *table, int n_classes, odr_ship_table **out) {
  REQUIRE(c && table && out, "NULL argument");
  REQUIRE(n_classes >= 1, "n_classes is %d, not positive", n_classes);
  const size_t n = (size_t)n_classes * SHIP_NTAB * 2;
  for (size_t k = 0; k < n; ++k) REQUIRE(table[k] == table[k], "NaN in the table of class %d", (int)(k / (SHIP_NTAB * 2)));
  double *d = nullptr;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMalloc((void **)&d, sizeof(double) * n));
  if (int rc = odr_i_h2d(c, d, table, sizeof(double) * n, c->stream)) { (void)hipFree(d); return rc; }
  *out = new odr_ship_table{d, n_classes};
  return 0;
}

int odr_ship_table_classes(const odr_ship_table *t, int32_t *n_classes) {
  REQUIRE(t && n_classes, "NULL argument");
  *n_classes = t->n_classes;
  return 0;
}

int odr_ship_table_destroy(odr_ctx *c, odr_ship_table *t) {
  REQUIRE(c, "NULL argument");
  if (!t) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));      // a launch that reads it may be in flight
  HIPCHK(hipFree(t->dev));
  delete t;
  return 0;
}

// ShipDrift.update (models/shipdrift.py:216-343) of every active element in ONE launch (odr_ship.hip.h).  Enqueued on the
// context's stream, no host synchronisation -- unless the caller asks for the float64 intermediates (10 n doubles on the host).
int odr_ship_drift(odr_ctx *c, odr_particles *p, int length_slot, int height_slot, int draft_slot, int beam_slot, int wind_drag_slot,
                   int water_drag_slot, int orientation_slot, int class_slot, const odr_ship_table *table, int hs_mode,
                   int tp_mode, int wave_dir_from_stokes, int stranded_code, double dt_seconds, double *intermediates_f64) {
  REQUIRE(c && p, "NULL argument");
  REQUIRE(dt_seconds == dt_seconds, "NaN argument");
  REQUIRE(table && table->dev && table->n_classes >= 1, "no class table");
  REQUIRE(stranded_code > 0, "stranded_code is %d: a stranded element must leave status 0 (active)", stranded_code);
  REQUIRE((hs_mode == 0 || hs_mode == 1) && (tp_mode == 0 || tp_mode == 3), "bad wave options (hs_mode 0 | 1, tp_mode 0 | 3)");
  if (!p->env[VAR_U] || !p->env[VAR_V]) return fail(ODR_ERR_STATE, "the current (x_sea_water_velocity, y_sea_water_velocity) must have been sampled");
  if (!p->env[VAR_XWIND] || !p->env[VAR_YWIND]) return fail(ODR_ERR_STATE, "the wind (x_wind, y_wind) must have been sampled");
  if (!p->env[VAR_LAND]) return fail(ODR_ERR_STATE, "land_binary_mask must have been sampled");
  if (wave_dir_from_stokes && (!p->env[VAR_SX] || !p->env[VAR_SY]))
    return fail(ODR_ERR_STATE, "the Stokes drift must have been sampled when wave_dir_from_stokes is set");
  if ((hs_mode == 0 && !p->env[VAR_HS]) || (tp_mode == 0 && !p->env[VAR_TP])) return fail(ODR_ERR_STATE, "Hs/Tp not sampled");
  if (int rc = property_slots(p, {length_slot, height_slot, draft_slot, beam_slot, wind_drag_slot, water_drag_slot, orientation_slot, class_slot}))
    return rc;
  p->epoch++;          // positions, status and moving change
  p->status_epoch++;   // (elements may be deactivated)
  if (p->n == 0) return 0;
  const ShipSlots S = {p->aux[length_slot], p->aux[height_slot], p->aux[draft_slot], p->aux[beam_slot], p->aux[wind_drag_slot],
                       p->aux[water_drag_slot], p->aux[orientation_slot], p->aux[class_slot]};
  double *report = nullptr;
  if (intermediates_f64) {
    void *base;
    if (int rc = scratch(c, p, sizeof(double) * 10 * (size_t)p->n, &base)) return rc;
    report = (double *)base;
  }
  if (report)
    hipLaunchKernelGGL(k_ship_drift<true>, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, view(p), S, table->dev, table->n_classes, hs_mode,
                       tp_mode, wave_dir_from_stokes != 0, stranded_code, dt_seconds, report);
  else
    hipLaunchKernelGGL(k_ship_drift<false>, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, view(p), S, table->dev, table->n_classes, hs_mode,
                       tp_mode, wave_dir_from_stokes != 0, stranded_code, dt_seconds, report);
  HIPCHK(hipGetLastError());
  if (report) D2H(intermediates_f64, report, sizeof(double) * 10 * (size_t)p->n);
  return 0;
}
