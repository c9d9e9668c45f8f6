// eg_breed.h — k_breed_gather, k_breed_turnover: what turns the survivors of a generation of plan crosses into the next generation's
// parents without a trip through the host (include/eirgrid_hip.h eg_breed_plans; the loop is csrc/eg_breed.cpp).  Included by
// eg_rollout.hip (eg_rollout.o only) behind eg_plan_crosses.h.
//
// A generation is evaluated in chunks.  Each chunk's variants are written by k_plan_crosses into the plan pool (block j = variant
// first + j: the routing of launch_plans permutes which workgroup runs which episode, never the blocks — k_rollout reads
// plan_pool + e * kPlanStride for the episode whose record is record e), replayed, and folded by the five kernels of eg_pareto.h into a
// PRIVATE archive (a ParetoState and its record slots, as eg_pareto_track's, in a buffer of the context's own: BreedLayout).  What the
// archive lacks is the plan: an entry names the record slot k_pareto_finalize gave it, and the pool is overwritten by the next chunk.
//   k_breed_gather    behind every chunk's fold: every entry whose index lies in [first, first + n) entered in this chunk (indices grow
//                     from chunk to chunk and a held entry keeps its index); its block, pool block index - first, is copied to BLOCK
//                     slot entry.slot.  A slot never moves while its entry is held, and a freed slot is overwritten by its next owner —
//                     the record slots' own rule.  The same grid counts the chunk's valid variants (eg_pareto_track's definition).
//   k_breed_turnover  once per generation: entry r of the archive (they stand in ascending index) has its block copied to position r of
//                     the OTHER parent array — k_plan_crosses read this generation's parents from the one, so no block is read after it
//                     has been overwritten, and the population of a generation without a valid variant still stands — and one readback
//                     row written: the entry (index = variant number, metrics, score, slot) and the block's two prefix-offset tables,
//                     from which the host enumerates and routes the next generation (breed::write_row).  The last workgroup to finish
//                     (breed::last_to_finish) empties the state and the counters for the next generation.
// ORDER.  A plan batch runs entirely on the null stream: launch_plans leaves RolloutPlan::stream_heavy null, so both replay variants
// (and k_replay_solo) are launched there, not on the side stream the training batches fork to.  k_plan_crosses, the replay grids, the
// five fold kernels, k_breed_gather and the next chunk's k_plan_crosses are therefore one in-order queue: the gather runs after the fold
// that assigned the slots and before the pool is written again, and k_breed_turnover after the last gather.  The host's copies (the
// packed crosses and the routing of the next chunk, the readback) are synchronous copies on the same stream.
// A wave per entry; vector loads and stores only, 16 bytes a lane; no LDS.  Every index read from memory is clamped, and a workgroup
// writes only inside its own block slot, parent position or readback row.
#pragma once

namespace breed {

using pblock::kOffOff;
constexpr int kVec = (int)(snap::kPlanStride / 16);      // 16-byte words of a plan block
static_assert(snap::kPlanStride % 16 == 0 && kOffOff % 16 == 0 && kBreedRowBytes == 64 + 2 * 4 * 28 && sizeof(ParetoEntry) == 56, "readback row layout");

__device__ __forceinline__ void copy_block(uint8_t* dst, const uint8_t* src, int lane) {
  const uint4* s = reinterpret_cast<const uint4*>(src);
  uint4* d = reinterpret_cast<uint4*>(dst);
  for (int w = lane; w < kVec; w += kWave) d[w] = s[w];
}

// a readback row: the entry in 8 words of 8 bytes (the last one padding), then the two offset tables of its block, 14 words of 16 bytes
__device__ __forceinline__ void write_row(uint8_t* row, const ParetoEntry* entry, const uint8_t* src_block, int lane) {
  if (lane < 8) reinterpret_cast<unsigned long long*>(row)[lane] = lane < 7 ? reinterpret_cast<const unsigned long long*>(entry)[lane] : 0ull;
  else if (lane < 8 + 14) reinterpret_cast<uint4*>(row + 64)[lane - 8] = reinterpret_cast<const uint4*>(src_block + kOffOff)[lane - 8];
}

// the tail of a turnover kernel (workgroups of one wave): whether this workgroup is the last to get here.  Then everybody has read the
// state and the counters (the fence stands between a workgroup's reads and its count), so the caller can empty what the next
// generation wants empty
__device__ __forceinline__ bool last_to_finish(BreedCounters* cnt, int lane) {
  __threadfence();
  unsigned t = 0u;
  if (lane == 0) t = atomicAdd(&cnt->done, 1u);
  t = (unsigned)__shfl((int)t, 0, kWave);
  return t == gridDim.x - 1u;
}

}  // namespace breed

// EG_PARETO_MAX workgroups of one wave: workgroup r looks at entry r; all of them together at the n records of the chunk
__global__ void __launch_bounds__(kWave) k_breed_gather(const ParetoState* st, DevOut O, uint32_t n, unsigned long long first, const uint8_t* __restrict__ pool,
                                                        uint8_t* __restrict__ blocks, BreedCounters* cnt) {
  const int lane = threadIdx.x & (kWave - 1), r = (int)blockIdx.x;
  const int held = pareto::clampi(st->n_held, 0, EG_PARETO_MAX);
  if (r < held && r < EG_PARETO_MAX) {
    const long long idx = st->e[r].index;
    if (idx >= (long long)first && (unsigned long long)idx - first < (unsigned long long)n) {
      const uint32_t j = (uint32_t)((unsigned long long)idx - first);
      const int slot = pareto::clampi(st->e[r].slot, 0, EG_PARETO_MAX - 1);
      breed::copy_block(blocks + (size_t)slot * snap::kPlanStride, pool + (size_t)j * snap::kPlanStride, lane);
    }
  }
  unsigned valid = 0;
  for (uint32_t e = blockIdx.x * (uint32_t)kWave + (uint32_t)lane; e < n; e += gridDim.x * (uint32_t)kWave) {
    if (*O.status(e) != EG_EP_OK) continue;
    const double* m = O.metrics(e);
    valid += (m[0] == m[0] && m[1] == m[1] && m[2] == m[2] && m[3] == m[3]) ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) valid += (unsigned)__shfl_xor((int)valid, o, kWave);
  if (lane == 0 && valid != 0u) atomicAdd(&cnt->n_valid, (unsigned long long)valid);
}

// EG_PARETO_MAX workgroups of one wave: workgroup r moves entry r
__global__ void __launch_bounds__(kWave) k_breed_turnover(ParetoState* st, const uint8_t* __restrict__ blocks, uint8_t* __restrict__ next_parents,
                                                          uint8_t* __restrict__ readback, BreedCounters* cnt) {
  const int lane = threadIdx.x & (kWave - 1), r = (int)blockIdx.x;
  const int held = pareto::clampi(st->n_held, 0, EG_PARETO_MAX);
  if (r < held && r < EG_PARETO_MAX) {
    const int slot = pareto::clampi(st->e[r].slot, 0, EG_PARETO_MAX - 1);
    const uint8_t* src = blocks + (size_t)slot * snap::kPlanStride;
    breed::copy_block(next_parents + (size_t)r * snap::kPlanStride, src, lane);
    breed::write_row(readback + kBreedHeaderBytes + (size_t)r * kBreedRowBytes, &st->e[r], src, lane);
  }
  if (r == 0 && lane == 0) {
    BreedHeader h;
    h.n_held = held; h.pad = 0; h.n_dropped = st->n_dropped; h.n_valid = (long long)cnt->n_valid; h.pad2 = 0;
    *reinterpret_cast<BreedHeader*>(readback) = h;
  }
  if (breed::last_to_finish(cnt, lane) && lane == 0) {      // the state and the counters, for the next generation
    st->n_held = 0; st->n_dropped = 0;
    cnt->n_valid = 0ull; cnt->done = 0u;
  }
}
