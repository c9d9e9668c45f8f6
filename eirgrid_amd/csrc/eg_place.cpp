// eg_place.cpp — single placement queries on the device: eg_place, eg_find_suitable_location.
#include "eg_host.h"

using namespace eg;

namespace {
// the queries' buffers (the generators' cells, the answer's cell and score), kept for the life of the context
int place_scratch(eg_ctx* c) {
  EG_HIP(c->d_place_cells.reserve(EG_MAX_GENS));
  EG_HIP(c->d_place_cell.reserve(1));
  EG_HIP(c->d_place_score.reserve(1));
  return EG_OK;
}
}  // namespace

extern "C" {

int32_t eg_place(eg_ctx* c, int32_t gen_type, int32_t year_index, const uint16_t* extra_cells, int32_t n_extra,
                 int32_t* out_cell, double* out_score) {
  if (!c || gen_type < 0 || gen_type >= EG_N_TYPES || year_index < 0 || year_index >= EG_YEARS || n_extra < 0 || n_extra > EG_ONCHIP_GENS) {
    set_error("eg_place: bad argument"); return EG_ERR_BAD_ARG;
  }
  for (int i = 0; i < n_extra; ++i) if (extra_cells[i] >= EG_CELLS) { set_error("eg_place: cell out of range"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_TRY(place_scratch(c));
  uint16_t* d_cells = c->d_place_cells; int32_t* d_cell = c->d_place_cell; double* d_score = c->d_place_score;
  if (n_extra) EG_HIP(hipMemcpy(d_cells, extra_cells, sizeof(uint16_t) * n_extra, hipMemcpyHostToDevice));
  EG_LAUNCH("k_place", launch_place(c->dev, gen_type, year_index, d_cells, n_extra, d_cell, d_score, nullptr));
  int32_t cell = -1; double score = 0.0;
  EG_HIP(hipMemcpy(&cell, d_cell, sizeof(cell), hipMemcpyDeviceToHost));
  EG_HIP(hipMemcpy(&score, d_score, sizeof(score), hipMemcpyDeviceToHost));
  if (out_cell) *out_cell = cell;
  if (out_score) *out_score = score;
  return EG_OK;
}

int32_t eg_find_suitable_location(eg_ctx* c, int32_t year_index, int32_t gen_type, const double* gen_x, const double* gen_y,
                                  int32_t n_generators, float size_penalty, double* out_x, double* out_y, int32_t* found, double* out_score) {
  if (!c || gen_type < 0 || gen_type >= EG_N_TYPES || year_index < 0 || year_index >= EG_YEARS || n_generators < 0 ||
      (n_generators > 0 && (!gen_x || !gen_y))) { set_error("eg_find_suitable_location: bad argument"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_TRY(place_scratch(c));
  EG_HIP(c->d_place_xy.reserve(2 * size_t(n_generators)));
  double* d_x = c->d_place_xy; double* d_y = d_x + c->d_place_xy.count / 2;      // (the buffer may be larger than this call needs)
  if (n_generators) {
    EG_HIP(hipMemcpy(d_x, gen_x, sizeof(double) * n_generators, hipMemcpyHostToDevice));
    EG_HIP(hipMemcpy(d_y, gen_y, sizeof(double) * n_generators, hipMemcpyHostToDevice));
  }
  const double radius = class_radius(c->tables.H.rclass[gen_type]);
  const double size_term = 1.0 - (double(size_penalty) * 0.1);                     // metal_location_search.rs:165
  EG_LAUNCH("k_place_xy", launch_place_xy(c->dev, gen_type, year_index, d_x, d_y, n_generators, radius, size_term, c->d_place_cell, c->d_place_score, nullptr));
  int32_t cell = -1; double score = 0.0;
  EG_HIP(hipMemcpy(&cell, c->d_place_cell, sizeof(cell), hipMemcpyDeviceToHost));
  EG_HIP(hipMemcpy(&score, c->d_place_score, sizeof(score), hipMemcpyDeviceToHost));
  if (found) *found = cell >= 0 ? 1 : 0;
  if (cell >= 0) { if (out_x) *out_x = double(cell / EG_GRID) * 1000.0; if (out_y) *out_y = double(cell % EG_GRID) * 1000.0; }
  if (out_score) *out_score = score;
  return EG_OK;
}

}  // extern "C"
