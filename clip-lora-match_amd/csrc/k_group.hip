// Grouped search (gfx950): the first k entries of a list that open a new group (clm_topk_distinct).
// A list holds (score, id, gid) entries already in the search order; an entry is kept iff no earlier
// list position carries its gid, entries with id < 0 (or gid < 0) are skipped, and the first k kept
// entries are written in list order, then (-inf, -1, -1).
//
// One workgroup of 256 threads walks one list in chunks of GC = 1024 entries (4 per thread, lane i at
// entry c0 + j * 256 + i: every load instruction of a wave reads consecutive addresses) and stops at
// k found. The gids seen so far live in an open-addressing table in LDS: GSLOTS = 4096 slots of
// (key i64, val u32), linear probing from a multiplicative hash of the full 64-bit gid. Keys are
// compared whole, so gids that share a slot (or every low bit) are still told apart.
//   val == 0         the gid was kept in an earlier chunk;
//   val == p + 1     the lowest position p of this chunk that carries the gid (atomicMin; a free slot
//                    holds 0xFFFFFFFF).
// Per chunk: (1) every live entry finds or claims its gid's slot (a 64-bit LDS compare-and-swap) and
// lowers val to its position + 1; (2) an entry is kept iff val == its position + 1 -- WHICH slot a gid
// got depends on the schedule, the minimum it holds does not, so the kept set is a pure function of
// the list; (3) a block prefix sum over the chunk's keep flags in position order gives each kept entry
// its output slot; (4) the kept entries are stored and their val set to 0. The table never holds more
// than k - 1 + GC < GSLOTS / 2 gids: a chunk is walked only while fewer than k were found, and the
// walk ends with the chunk that reaches k. LDS: 32 KiB keys + 16 KiB vals + 4 KiB flags = 52 KiB, so
// two workgroups share a CU.
#include <algorithm>

#include "kernels.hpp"

namespace clm {

namespace {

constexpr int GT = 256;        // threads per workgroup
constexpr int GPER = 4;        // entries per thread and chunk
constexpr int GC = GT * GPER;  // entries per chunk
constexpr int GSLOTS = 4096;   // table slots (a power of two, > 2 * (1024 - 1 + GC))
constexpr int GSHIFT = 64 - 12;
static_assert((1 << (64 - GSHIFT)) == GSLOTS, "the hash keeps log2(GSLOTS) bits");
constexpr unsigned long long GEMPTY = ~0ull;   // no gid >= 0 has this pattern

__device__ __forceinline__ unsigned slot_of(unsigned long long gid) {
  return (unsigned)((gid * 0x9E3779B97F4A7C15ull) >> GSHIFT);
}

// the exclusive prefix sum of v over the 256 threads; lds: 4 ints; *total: the block's sum
__device__ __forceinline__ unsigned block_exclusive(unsigned v, unsigned* lds, unsigned* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = (unsigned)__shfl_up((int)inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  unsigned base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < w) base += lds[i];
    tot += lds[i];
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(GT) void topk_distinct_kernel(const float* __restrict__ in_s,
                                                           const int64_t* __restrict__ in_i,
                                                           const int64_t* __restrict__ in_g,
                                                           const int64_t* __restrict__ offsets, int64_t ld, int64_t nq,
                                                           int k, float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                           int64_t* __restrict__ out_g, int* __restrict__ out_found) {
  __shared__ unsigned long long keys[GSLOTS];
  __shared__ unsigned vals[GSLOTS];
  __shared__ unsigned flag[GC];   // keep flag of each chunk position, then its exclusive rank
  __shared__ unsigned part[4];
  const volatile unsigned long long* vkeys = keys;   // probes read what other waves have claimed
  const volatile unsigned* vvals = vals;
  const int t = threadIdx.x;

  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    int64_t begin = q * ld, len = ld;
    if (offsets) {
      begin = offsets[q];
      len = offsets[q + 1] - begin;
    }
    if (len < 0) len = 0;
    for (int s = t; s < GSLOTS; s += GT) {
      keys[s] = GEMPTY;
      vals[s] = 0xFFFFFFFFu;
    }
    __syncthreads();

    int found = 0;
    for (int64_t c0 = 0; c0 < len && found < k; c0 += GC) {
      const int m = (int)std::min<int64_t>(GC, len - c0);
      float sc[GPER];
      int64_t id[GPER], gid[GPER];
      int slot[GPER];
#pragma unroll
      for (int j = 0; j < GPER; ++j) {
        const int p = j * GT + t;
        slot[j] = -1;
        id[j] = -1;
        gid[j] = -1;
        sc[j] = 0.0f;
        if (p < m) {
          id[j] = in_i[begin + c0 + p];
          gid[j] = in_g[begin + c0 + p];
          sc[j] = in_s[begin + c0 + p];
        }
        if (id[j] >= 0 && gid[j] >= 0) {
          const unsigned long long g = (unsigned long long)gid[j];
          unsigned s = slot_of(g);
          for (;;) {   // ends: fewer than GSLOTS / 2 gids are ever in the table
            unsigned long long cur = vkeys[s];
            if (cur == GEMPTY) {
              cur = atomicCAS(&keys[s], GEMPTY, g);
              if (cur == GEMPTY) cur = g;   // claimed
            }
            if (cur == g) break;
            s = (s + 1) & (GSLOTS - 1);
          }
          slot[j] = (int)s;
          // 0 = kept by an earlier chunk, and stays 0 throughout this phase
          if (vvals[s] != 0u) atomicMin(&vals[s], (unsigned)p + 1u);
        }
      }
      __syncthreads();   // every gid of the chunk holds its lowest position + 1
      bool keep[GPER];
#pragma unroll
      for (int j = 0; j < GPER; ++j) {
        const int p = j * GT + t;
        keep[j] = slot[j] >= 0 && vals[slot[j]] == (unsigned)p + 1u;
        flag[p] = keep[j] ? 1u : 0u;
      }
      __syncthreads();
      // ranks in position order: thread t sums positions 4 t .. 4 t + 3
      unsigned f[GPER], mine = 0;
#pragma unroll
      for (int j = 0; j < GPER; ++j) {
        f[j] = flag[t * GPER + j];
        mine += f[j];
      }
      unsigned total = 0;
      unsigned run = block_exclusive(mine, part, &total);   // (its barriers also order the reads above)
#pragma unroll
      for (int j = 0; j < GPER; ++j) {
        flag[t * GPER + j] = run;
        run += f[j];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < GPER; ++j) {
        if (!keep[j]) continue;
        vals[slot[j]] = 0u;
        const int64_t o = (int64_t)found + flag[j * GT + t];
        if (o < k) {
          out_s[q * k + o] = sc[j];
          out_i[q * k + o] = id[j];
          out_g[q * k + o] = gid[j];
        }
      }
      found += (int)total;
      __syncthreads();   // flag and vals are rewritten by the next chunk
    }
    found = std::min(found, k);
    for (int o = found + t; o < k; o += GT) {
      out_s[q * k + o] = -__builtin_inff();
      out_i[q * k + o] = -1;
      out_g[q * k + o] = -1;
    }
    if (t == 0) out_found[q] = found;
    __syncthreads();   // the table is cleared for the next list
  }
}

}  // namespace

hipError_t topk_distinct(const float* in_s, const int64_t* in_i, const int64_t* in_g, const int64_t* offsets,
                         int64_t ld, int64_t nq, int k, float* out_s, int64_t* out_i, int64_t* out_g, int* out_found,
                         hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (k < 1 || k > 1024 || ld < 0) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)std::min<int64_t>(nq, 1 << 16);
  topk_distinct_kernel<<<grid, GT, 0, s>>>(in_s, in_i, in_g, offsets, ld, nq, k, out_s, out_i, out_g, out_found);
  return hipGetLastError();
}

}  // namespace clm
