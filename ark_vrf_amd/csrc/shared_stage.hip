// shared_stage.hip -- the suite-independent staging of a Thin or Pedersen batch over a table of shared points (thin_shared.h): the plain staged
// layout gathered from the table, and the counting sort of the references by row (32-bit integer atomics on counters only).  Thin: n keys
// and tot_io inputs; Pedersen: the tot_io inputs alone (n = 0 here, and a batch whose items have no pairs leaves every row unreferenced).
// A segmented run over such a staging sorts the same references once more, by (segment, row): shared_seg_plan.
#include "thin_shared.h"
#include "thin_seg.h"
#include "fpn.h"

namespace avrf {

// ---------------------------------------------------------------- staging: gather and plan

// ctr[r] += 1 for every active lane, returning the value each lane's own increment saw.  References crowd on few rows (a handful of
// inputs, one key), and same-address atomics serialise: the lanes of a wave that name the row of the wave's first pending lane are
// counted with ONE atomic, four times over; what is still pending after that (rows that differ lane by lane) goes one by one.
AVRF_DI uint32_t wave_count(uint32_t *ctr, uint32_t r, bool active) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t slot = 0;
  bool todo = active;
  for (int round = 0; round < 4; round++) {
    const unsigned long long pending = __ballot(todo);
    if (!pending) break;                                                // (wave-uniform)
    const int leader = __ffsll(pending) - 1;
    const uint32_t key = __shfl(r, leader);
    const bool mine = todo && r == key;
    const unsigned long long m = __ballot(mine);
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(ctr + key, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    if (mine) { slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1)); todo = false; }
  }
  if (todo) slot = atomicAdd(ctr + r, 1u);
  return slot;
}

// reference t: item t's key (t < n) or the input of I/O pair t - n.  Copies the row (and the pair's output) into the plain staged
// layout and counts the reference of its row.
__global__ void __launch_bounds__(256)
k_shared_gather(const uint8_t *__restrict__ table, uint32_t n_shared, const uint32_t *__restrict__ idx, const uint8_t *__restrict__ outs,
                uint32_t n, uint32_t tot_io, uint8_t *__restrict__ pks, uint8_t *__restrict__ ios, uint32_t *__restrict__ cnt) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < n + tot_io;
  uint32_t r = active ? idx[t] : 0;
  if (r >= n_shared) r = n_shared - 1;                                  // (refused on the host; never a read outside the table)
  wave_count(cnt, r, active);
  if (!active) return;
  const uint4 *src = reinterpret_cast<const uint4 *>(table + 64 * (size_t)r);
  uint4 *dst = reinterpret_cast<uint4 *>(t < n ? pks + 64 * (size_t)t : ios + 128 * (size_t)(t - n));
#pragma unroll
  for (int i = 0; i < 4; i++) dst[i] = src[i];
  if (t >= n) {
    const uint4 *o = reinterpret_cast<const uint4 *>(outs + 64 * (size_t)(t - n));
#pragma unroll
    for (int i = 0; i < 4; i++) dst[4 + i] = o[i];
  }
}

// exclusive prefix sums of the counts (one block; every thread a contiguous chunk): row_off[0 .. T], and the counts replaced by
// the same offsets as the placement's cursors
__global__ void __launch_bounds__(1024)
k_shared_scan(uint32_t *__restrict__ cursor, uint32_t *__restrict__ row_off, uint32_t n_shared) {
  __shared__ uint32_t sums[1024];
  const uint32_t tid = threadIdx.x, chunk = (n_shared + 1023) / 1024;
  const uint32_t lo = tid * chunk < n_shared ? tid * chunk : n_shared, hi = lo + chunk < n_shared ? lo + chunk : n_shared;
  uint32_t s = 0;
  for (uint32_t i = lo; i < hi; i++) s += cursor[i];
  sums[tid] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint32_t v = tid >= d ? sums[tid - d] : 0;
    __syncthreads();
    sums[tid] += v;
    __syncthreads();
  }
  uint32_t base = sums[tid] - s;
  for (uint32_t i = lo; i < hi; i++) { const uint32_t c = cursor[i]; row_off[i] = base; cursor[i] = base; base += c; }
  if (tid == 1023) row_off[n_shared] = sums[1023];
}

__global__ void __launch_bounds__(256)
k_shared_place(const uint32_t *__restrict__ idx, uint32_t n_shared, uint32_t n_contrib, uint32_t *__restrict__ cursor,
               uint32_t *__restrict__ pos, uint32_t *__restrict__ slot_row) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < n_contrib;
  uint32_t r = active ? idx[t] : 0;
  if (r >= n_shared) r = n_shared - 1;
  const uint32_t s = wave_count(cursor, r, active);                     // < row_off[r + 1] <= n_contrib: the same references were counted
  if (active) { pos[t] = s; slot_row[s] = r; }
}

hipError_t shared_plan(const uint8_t *d_table, uint32_t n_shared, const uint32_t *d_idx, const uint8_t *d_outputs, uint32_t n, uint32_t tot_io,
                       uint8_t *d_pks, uint8_t *d_ios, uint32_t *d_plan, hipStream_t st) {
  const uint32_t nc = n + tot_io;
  if (!n_shared) return hipSuccess;
  uint32_t *cursor = d_plan, *row_off = d_plan + (n_shared + 1), *pos = row_off + (n_shared + 1), *slot_row = pos + nc;
  if (hipError_t e = hipMemsetAsync(cursor, 0, (size_t)(n_shared + 1) * 4, st)) return e;
  if (nc) hipLaunchKernelGGL(k_shared_gather, dim3((nc + 255) / 256), dim3(256), 0, st, d_table, n_shared, d_idx, d_outputs, n, tot_io, d_pks, d_ios, cursor);
  hipLaunchKernelGGL(k_shared_scan, dim3(1), dim3(1024), 0, st, cursor, row_off, n_shared);
  if (nc) hipLaunchKernelGGL(k_shared_place, dim3((nc + 255) / 256), dim3(256), 0, st, d_idx, n_shared, nc, cursor, pos, slot_row);
  return hipGetLastError();                                             // (a launch that was refused)
}

// ---------------------------------------------------------------- the plan of one segmented run (thin_shared.h shared_seg_plan)

// reference t (as above) -> its virtual row v T + row: v the segment of its item -- item t for a key, the item of I/O pair t - nk for an
// input (both by the search of thin_seg.h) -- and the histogram of the virtual rows
__global__ void __launch_bounds__(256)
k_shared_seg_rows(const uint32_t *__restrict__ idx, const uint32_t *__restrict__ io_off, const uint32_t *__restrict__ seg_off, uint32_t n_seg,
                  uint32_t n_shared, uint32_t n, uint32_t nk, uint32_t tot_io, uint32_t *__restrict__ vrow, uint32_t *__restrict__ cnt) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < nk + tot_io;
  uint32_t row = 0;
  if (active) {
    uint32_t r = idx[t];
    if (r >= n_shared) r = n_shared - 1;                                // (refused on the host; never a row outside the histogram)
    const uint32_t j = t < nk ? t : segment_of(io_off, n, t - nk);
    row = segment_of(seg_off, n_seg, j) * n_shared + r;
    vrow[t] = row;
  }
  wave_count(cnt, row, active);
}

hipError_t shared_seg_plan(const uint32_t *d_idx, const uint32_t *d_io_off, const uint32_t *d_seg_off, uint32_t n_seg, uint32_t n_shared, uint32_t n,
                           uint32_t nk, uint32_t tot_io, uint32_t *d_plan, hipStream_t st) {
  const uint32_t nc = nk + tot_io, rows = n_seg * n_shared;
  if (!rows) return hipSuccess;
  uint32_t *cursor = d_plan, *row_off = d_plan + (rows + 1), *pos = row_off + (rows + 1), *slot_row = pos + nc, *vrow = slot_row + nc;
  if (hipError_t e = hipMemsetAsync(cursor, 0, (size_t)(rows + 1) * 4, st)) return e;
  if (nc) hipLaunchKernelGGL(k_shared_seg_rows, dim3((nc + 255) / 256), dim3(256), 0, st, d_idx, d_io_off, d_seg_off, n_seg, n_shared, n, nk, tot_io, vrow, cursor);
  hipLaunchKernelGGL(k_shared_scan, dim3(1), dim3(1024), 0, st, cursor, row_off, rows);
  if (nc) hipLaunchKernelGGL(k_shared_place, dim3((nc + 255) / 256), dim3(256), 0, st, vrow, rows, nc, cursor, pos, slot_row);
  return hipGetLastError();
}

}  // namespace avrf
