// eg_device_tables.h — the device table blob as a function of the host tables (eg_device_tables.cpp; plain C++, no HIP).
#pragma once
#include "eg_internal.h"

namespace eg {
// what eg_create takes from the construction besides the bytes
struct BlobInfo {
  int n_variants = 0;               // distinct (radius class, marine) pairs over the types
  bool box_list_fits = false;       // the heavy episodes' box list holds every entry (else heavy episodes keep the exact scan)
  bool hoist_supported = false;     // the hoisted replay is sized for this world's radii / variants
};

// The tab:: layout of eg_internal.h, filled from H (blob is resized to tab::total).  EG_OK, or EG_ERR_BAD_ARG with the error text set.
int build_device_blob(const HostTables& H, std::vector<uint8_t>& blob, BlobInfo& info);
}  // namespace eg
