// eg_device_tables.cpp — the device table blob (eg_internal.h tab::) from the host tables: the tables themselves, the sorted
// candidate lists and their ranks, the tile bounds of place_tiles, the compact factor table, the heavy episodes' box lists.
// No HIP here: plain C++ with eg_tables.cpp's flags (csrc/Makefile), so that the doubles are the ones eg_tables.cpp would make.
#include "eg_device_tables.h"

#include <algorithm>
#include <cstring>

namespace eg {
namespace {
template <typename T>
void put(std::vector<uint8_t>& blob, size_t off, const std::vector<T>& v, size_t max_count) {
  const size_t n = v.size() < max_count ? v.size() : max_count;
  if (n) std::memcpy(blob.data() + off, v.data(), sizeof(T) * n);
}
}  // namespace

int build_device_blob(const HostTables& H, std::vector<uint8_t>& blob, BlobInfo& info) {
  blob.assign(tab::total, 0);
  put(blob, tab::usage, H.usage, kYears); put(blob, tab::population, H.population, kYears);
  put(blob, tab::pre_co2, H.pre_co2, kYears); put(blob, tab::pre_tg, H.pre_tg, kYears); put(blob, tab::pre_ig, H.pre_ig, kYears);
  put(blob, tab::pre_sg, H.pre_sg, kYears); put(blob, tab::pre_optot, H.pre_optot, kYears); put(blob, tab::pre_opcnt, H.pre_opcnt, kYears);
  put(blob, tab::inflation, H.inflation, kYears); put(blob, tab::carbon_price, H.carbon_price, kYears);
  put(blob, tab::out_mw, H.out_mw, kTypes); put(blob, tab::co2_t, H.co2_t, kTypes);
  put(blob, tab::cls, H.cls, kTypes); put(blob, tab::rclass, H.rclass, kTypes); put(blob, tab::marine, H.marine, kTypes);
  put(blob, tab::reach, H.reach, kRadiusClasses);
  put(blob, tab::dr, H.dr, size_t(kRadiusClasses) * 169); put(blob, tab::m03, H.m03, kCells); put(blob, tab::t12, H.t12, size_t(kYears) * kTypes);
  put(blob, tab::offv, H.offv, size_t(kYears) * kOffsetTypes * kYears); put(blob, tab::offc, H.offc, size_t(kYears) * kOffsetTypes * kMults);
  put(blob, tab::cc, H.cc, size_t(kYears) * kTypes * kYears * kMults * 2);
  put(blob, tab::te_cell, H.te, size_t(kYears) * kRadiusClasses * kCells); put(blob, tab::coastf, H.coastf, kCells);
  {  // Sorted candidate lists.  final(c) = ((te[c] * prod_g d/R) * cf[c]) * size <= base(c) = (te[c] * cf[c]) * size
     // because every factor is in [0, 1] and IEEE multiplication is monotone, so a scan in descending base order can
     // stop as soon as the next base is below the best final score found (k_rollout / place_search).
    std::vector<std::pair<int, int>> variants;   // (radius class, marine)
    std::vector<int32_t> variant_of(kTypes, 0);
    for (int t = 0; t < kTypes; ++t) {
      std::pair<int, int> key(H.rclass[t], H.marine[t] ? 1 : 0);
      size_t v = 0;
      while (v < variants.size() && variants[v] != key) ++v;
      if (v == variants.size()) variants.push_back(key);
      variant_of[t] = int32_t(v);
    }
    const int NV = int(variants.size());
    if (NV > kMaxVariants) { set_error("eg_create: too many (radius class, marine) variants"); return EG_ERR_BAD_ARG; }
    put(blob, tab::variant, variant_of, kTypes);
    info.n_variants = NV;
    PsRec* ps = reinterpret_cast<PsRec*>(blob.data() + tab::ps);   // entries beyond the 2601 candidates stay te = 0
    std::vector<double> base(kCells);
    std::vector<int> order(kCells);
    for (int y = 0; y < kYears; ++y)
      for (int v = 0; v < NV; ++v) {
        const double* te = &H.te[(size_t(y) * kRadiusClasses + variants[v].first) * kCells];
        const bool marine = variants[v].second != 0;
        for (int c2 = 0; c2 < kCells; ++c2) { base[c2] = (te[c2] * (marine ? H.coastf[c2] : 1.0)) * H.size_factor; order[c2] = c2; }
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return base[a] > base[b]; });
        PsRec* list = ps + (size_t(y) * kMaxVariants + v) * kPsStride;
        for (int r = 0; r < kPsStride; ++r) { list[r].te = 0.0; list[r].cf = 1.0; list[r].m03 = 0.0; list[r].cell = 0; list[r].pad = 0; }
        double* pb = reinterpret_cast<double*>(blob.data() + tab::pbase) + (size_t(y) * kMaxVariants + v) * kPcStride;
        uint32_t* pc = reinterpret_cast<uint32_t*>(blob.data() + tab::pcell) + (size_t(y) * kMaxVariants + v) * kPcStride;
        for (int r = 0; r < kPcStride; ++r) { pb[r] = r < kCells ? base[order[r]] : 0.0; pc[r] = r < kCells ? uint32_t(order[r]) : 0u; }
        std::memcpy(blob.data() + tab::cbase + 8 * (size_t(y) * kMaxVariants + v) * kCells, base.data(), 8 * size_t(kCells));      // the same scores per cell
        uint16_t* rank = reinterpret_cast<uint16_t*>(blob.data() + tab::crank) + (size_t(y) * kMaxVariants + v) * kCells;      // ... their ranks
        for (int r = 0; r < kCells; ++r) rank[order[r]] = uint16_t(r);
        for (int r = 0; r < kCells; ++r) {
          list[r].te = te[order[r]]; list[r].cf = marine ? H.coastf[order[r]] : 1.0; list[r].m03 = H.m03[order[r]]; list[r].cell = uint32_t(order[r]);
          list[r].pad = uint32_t(4 * (order[r] / kGrid)) | (uint32_t(4 * (order[r] % kGrid)) << 16);
        }
      }
  }
  {  // the tile bounds of place_tiles (eg_internal.h tab::ucell): score(y, c) * field(c) = (score(y, c) / u(c)) * (u(c) * field(c)),
     // at most the tile's largest ratio times a bound of u * field on the tile (the ratio rounded up by 2^-40: far more than
     // the few roundings in between)
    const double* cb = reinterpret_cast<const double*>(blob.data() + tab::cbase);
    double* uc = reinterpret_cast<double*>(blob.data() + tab::ucell);
    double* um = reinterpret_cast<double*>(blob.data() + tab::umax);
    double* rm = reinterpret_cast<double*>(blob.data() + tab::rmax);
    auto tile_of = [](int c2) { return (c2 / kGrid / kTileW) * kTileCols + (c2 % kGrid) / kTileW; };
    for (int v = 0; v < info.n_variants; ++v) {
      double* u = uc + size_t(v) * kCells;
      for (int c2 = 0; c2 < kCells; ++c2)
        for (int y = 0; y < kYears; ++y) u[c2] = std::max(u[c2], cb[(size_t(y) * kMaxVariants + v) * kCells + c2]);
      for (int c2 = 0; c2 < kCells; ++c2) um[size_t(v) * 64 + tile_of(c2)] = std::max(um[size_t(v) * 64 + tile_of(c2)], u[c2]);
      for (int y = 0; y < kYears; ++y) {
        double* r = rm + (size_t(y) * kMaxVariants + v) * 64;
        for (int c2 = 0; c2 < kCells; ++c2)
          if (u[c2] >= 1e-300) r[tile_of(c2)] = std::max(r[tile_of(c2)], cb[(size_t(y) * kMaxVariants + v) * kCells + c2] / u[c2]);
        for (int t = 0; t < kTiles; ++t) r[t] = r[t] * (1.0 + 0x1p-40);
      }
    }
  }
  {  // compact factor table (eg_rollout.hip load_factor_table): class k keeps squared distances 0..cap_k, cap_k = the first at which
     // the factor is 1.0 (d >= R); the factor must depend on the squared distance only and reach 1.0 within 12 cells
    int32_t* meta = reinterpret_cast<int32_t*>(blob.data() + tab::dr_meta);
    int next = 0;
    for (int k = 0; k < kRadiusClasses; ++k) {
      int cap = 1 << 30;
      for (int ai = 0; ai <= kMaxReach; ++ai) for (int aj = 0; aj <= kMaxReach; ++aj)
        if (H.dr[(size_t(k) * 13 + ai) * 13 + aj] == 1.0 && ai * ai + aj * aj < cap) cap = ai * ai + aj * aj;
      bool radial = cap <= kMaxReach * kMaxReach;
      for (int ai = 0; ai <= kMaxReach && radial; ++ai) for (int aj = 0; aj <= kMaxReach; ++aj)
        if ((H.dr[(size_t(k) * 13 + ai) * 13 + aj] == 1.0) != (ai * ai + aj * aj >= cap)) { radial = false; break; }
      if (!radial || cap > 255) { set_error("eg_create: the distance factors of a radius class are not a function of the squared distance that reaches 1.0 within 12 cells"); return EG_ERR_BAD_ARG; }
      meta[k] = next; meta[8 + k] = cap;
      next += (cap + 1 + 1) & ~1;      // entries 0..cap, every class starts at an even entry
    }
    if (next > kDrCompact) { set_error("eg_create: radii too large for the compact factor table"); return EG_ERR_BAD_ARG; }
    {      // the table as the kernels hold it in LDS (eg_rollout.hip load_factor_table copies it)
      double* drc = reinterpret_cast<double*>(blob.data() + tab::dr_compact);
      for (int i = 0; i < kDrCompact; ++i) drc[i] = 1.0;
      for (int k = 0; k < kRadiusClasses; ++k)
        for (int ai = 0; ai <= kMaxReach; ++ai) for (int aj = 0; aj <= kMaxReach; ++aj) {
          const int q = ai * ai + aj * aj;
          if (q < meta[8 + k]) drc[meta[k] + q] = H.dr[(size_t(k) * 13 + ai) * 13 + aj];
        }
    }
  }
  {  // heavy episodes (eg_field.h heavy_add): every (class, di, dj) with a factor below 1, i.e. closer than the class radius
    uint32_t* box = reinterpret_cast<uint32_t*>(blob.data() + tab::hv_box);
    int nbox = 0;
    for (int k = 0; k < kRadiusClasses; ++k)
      for (int di = -kMaxReach; di <= kMaxReach; ++di)
        for (int dj = -kMaxReach; dj <= kMaxReach; ++dj) {
          const int ai = di < 0 ? -di : di, aj = dj < 0 ? -dj : dj;
          if (H.dr[(size_t(k) * 13 + ai) * 13 + aj] == 1.0) continue;
          if (nbox < 1024) box[nbox] = uint32_t(di + 16) | (uint32_t(dj + 16) << 5) | (uint32_t(di * di + dj * dj) << 10) | (uint32_t(k) << 19);
          ++nbox;
        }
    info.box_list_fits = nbox <= 1024;      // radii the list was not sized for: heavy episodes keep the exact scan
    // (the hoisted replay updates its field with one lane per entry of this list and keeps the scores of eight variants in registers)
    info.hoist_supported = nbox <= 1024 && info.n_variants <= 8;
    for (int i = nbox; i < 1024; ++i) box[i] = 145u << 10;      // padding: class 0, di = dj = -16 (no class reaches that far), q = 145 (factor 1.0)
    for (int k = 0, i = 0; k <= kRadiusClasses; ++k) {      // words 1024..1030: where class k starts (the list is sorted by class), then the end
      while (i < nbox && i < 1024 && int(box[i] >> 19) < k) ++i;
      box[1024 + k] = uint32_t(i);
    }
    // ... and packed for every subset of classes, in the throughput kernel's form (tab::hv_lists): the long-replay variant reads its
    // subset's list from here (a few KB that every long replay of a CU shares) instead of keeping 4 KB of LDS for a copy of its own
    if (nbox <= 1024) {
      const int32_t* meta = reinterpret_cast<const int32_t*>(blob.data() + tab::dr_meta);
      uint32_t* lists = reinterpret_cast<uint32_t*>(blob.data() + tab::hv_lists);
      int32_t* quads = reinterpret_cast<int32_t*>(blob.data() + tab::hv_quads);
      auto place = [&](uint32_t en) -> uint32_t {
        const int k = int(en >> 19), q = int((en >> 10) & 511u);
        return (en & ~(511u << 10)) | (uint32_t(meta[k] + std::min(q, meta[8 + k])) << 10);
      };
      for (int mask = 0; mask < 64; ++mask) {
        uint32_t* l = lists + size_t(mask) * 1024;
        int n = 0;
        for (int k = 0; k < kRadiusClasses; ++k)
          if ((mask >> k) & 1) for (uint32_t i = box[1024 + k]; i < box[1024 + k + 1]; ++i) l[n++] = place(box[i]);
        const int padded = (n + 255) & ~255;
        for (int i = n; i < 1024; ++i) l[i] = place(145u << 10);
        quads[mask] = padded / 256;
      }
    }
  }
  return EG_OK;
}

}  // namespace eg
