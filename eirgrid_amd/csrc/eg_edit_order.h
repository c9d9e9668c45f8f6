// eg_edit_order.h — the canonical order of a plan's one-entry edits (include/eirgrid_hip.h eg_evaluate_plan_edits, eg_refine_plan), the one
// engine.py::sensitivity_edits / refine_edits build: none; every entry of list 0 (best_actions), then of list 1 (best_deficit_actions), deleted,
// in (year, position) order; every list-0 entry replaced by each action of `replace`; with `appends`, each action of `append` appended to each
// year's list 0.  count0 / count1: the EG_YEARS per-year lengths of the two lists.
#pragma once
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
}  // namespace eg
