// eg_edit_order.h — the canonical order of a plan's one-entry edits (include/eirgrid_hip.h eg_evaluate_plan_edits, eg_refine_plan) and, at the
// end of the file, of its moves.  The edits' order is the one
// engine.py::sensitivity_edits / refine_edits build: none; every entry of list 0 (best_actions), then of list 1 (best_deficit_actions), deleted,
// in (year, position) order; every list-0 entry replaced by each action of `replace`; with `appends`, each action of `append` appended to each
// year's list 0.  count0 / count1: the EG_YEARS per-year lengths of the two lists.
#pragma once
#include <algorithm>
#include <vector>

#include "eirgrid_hip.h"

namespace eg {
inline void enumerate_edits(const int32_t* count0, const int32_t* count1, const uint8_t* replace, int32_t n_replace, const uint8_t* append, int32_t n_append,
                            bool appends, std::vector<eg_plan_edit>& edits) {
  const int32_t* count[2] = {count0, count1};
  edits.assign(1, eg_plan_edit{EG_EDIT_NONE, 0, 0, 0, 0});
  for (int w = 0; w < 2; ++w)
    for (int y = 0; y < EG_YEARS; ++y)
      for (int32_t i = 0; i < count[w][y]; ++i) edits.push_back(eg_plan_edit{EG_EDIT_DELETE, uint8_t(w), uint16_t(y), uint32_t(i), 0});
  for (int y = 0; y < EG_YEARS; ++y)
    for (int32_t i = 0; i < count0[y]; ++i)
      for (int32_t k = 0; k < n_replace; ++k) edits.push_back(eg_plan_edit{EG_EDIT_REPLACE, 0, uint16_t(y), uint32_t(i), replace[k]});
  for (int y = 0; appends && y < EG_YEARS; ++y)
    for (int32_t k = 0; k < n_append; ++k) edits.push_back(eg_plan_edit{EG_EDIT_INSERT, 0, uint16_t(y), uint32_t(count0[y]), append[k]});
}
// The move variants of a refinement round (include/eirgrid_hip.h eg_refine_plans_moves), the order engine.py::refine_moves builds: every
// entry of list 0 in (year, position) order, and per entry each shift d = -1, +1, -2, +2, ..., -max_shift, +max_shift with 0 <= year + d
// <= 25: the entry moved behind the last entry of year year + d.
inline void enumerate_moves(const int32_t* count0, int32_t max_shift, std::vector<eg_plan_move>& moves) {
  moves.clear();
  for (int y = 0; y < EG_YEARS; ++y)
    for (int32_t i = 0; i < count0[y]; ++i)
      for (int32_t s = 1; s <= max_shift; ++s)
        for (int d : {-s, s})
          if (y + d >= 0 && y + d < EG_YEARS) moves.push_back(eg_plan_move{0, uint8_t(y + d), uint16_t(y), uint32_t(i), uint32_t(count0[y + d])});
}
// ... and how many they are
inline int64_t count_moves(const int32_t* count0, int32_t max_shift) {
  int64_t n = 0;
  for (int y = 0; y < EG_YEARS; ++y) n += int64_t(count0[y]) * (std::min<int>(max_shift, y) + std::min<int>(max_shift, EG_YEARS - 1 - y));
  return n;
}
}  // namespace eg
