// pb_select.hip -- pb_slot_select's kernel: a per-filter masked copy of one whole state array into another.
//
// The state array is tiled (rbis_device.hpp): a tile of 64 filters is NROW rows of 64 x 16 bytes, row r holding the
// component pair (slot 2r, slot 2r+1) of each filter.  One lane = one filter, so a lane's 16-byte access (global_load/store_dwordx4)
// moves two components of ITS filter and a wave instruction moves one contiguous 1 KiB row.  The mask is read once per lane; a lane
// whose filter is not selected leaves before its first state access, so a tile with nothing selected moves no state bytes (its wave
// reads 64 mask bytes and ends).  Lanes past the batch (the ragged last tile) count as not selected.  A workgroup is one wave on
// SEL_ROWS consecutive rows of one tile (grid: tiles x row chunks; the last chunk of a tile holds the NROW % SEL_ROWS remaining rows):
// the chunk's rows are staged in VGPRs (no scratch: `make resource-usage`), and the ISA issues 12 of its 16 loads before its first wait
// and keeps up to 16 in flight while it stores the rows that have arrived (16 KiB per wave).
#include "pb_ctx.hpp"

namespace {

constexpr int SEL_ROWS = 16;

// R rows starting at row r0 of the lane's column (the array stays in VGPRs: its indices are compile-time constants and no element is
// guarded -- a run-time guard per element put the whole array in scratch)
template <int R>
__device__ __forceinline__ void copy_rows(double2 *__restrict__ d2, const double2 *__restrict__ s2, int r0)
{
  double2 v[R];
#pragma unroll
  for (int i = 0; i < R; i++) v[i] = s2[(size_t) (r0 + i) * 64];
#pragma unroll
  for (int i = 0; i < R; i++) d2[(size_t) (r0 + i) * 64] = v[i];
}

template <int NS>
__global__ __launch_bounds__(64) void k_slot_select(double *__restrict__ dst, const double *__restrict__ src, const uint8_t *__restrict__ mask,
                                                    int B, int when)
{
  using S = Slots<NS>;
  static_assert(S::TILE == 64, "one lane per filter of a tile");
  constexpr int TAIL = S::NROW % SEL_ROWS;   // rows of the last chunk when NROW is not a multiple of SEL_ROWS (70 -> 6, 129 -> 1)
  const int lane = threadIdx.x;
  const long b = (long) blockIdx.x * S::TILE + lane;
  if (b >= B) return;
  if ((mask[b] != 0) != (when != 0)) return;
  const int r0 = blockIdx.y * SEL_ROWS;
  const size_t base = (size_t) blockIdx.x * S::TILE_DOUBLES + (size_t) lane * 2;
  const double2 *s2 = reinterpret_cast<const double2 *>(src + base);
  double2 *d2 = reinterpret_cast<double2 *>(dst + base);
  if (TAIL == 0 || r0 + SEL_ROWS <= S::NROW) copy_rows<SEL_ROWS>(d2, s2, r0);
  else copy_rows<(TAIL > 0 ? TAIL : 1)>(d2, s2, r0);   // the last chunk: rows [NROW - TAIL, NROW)
}

}  // namespace

int pbk_slot_select(pb_ctx *c, double *dst, const double *src, const uint8_t *mask_dev, int when)
{
  const dim3 grid((unsigned) nblk(c->B), (unsigned) (((c->ns == 15 ? Slots<15>::NROW : Slots<21>::NROW) + SEL_ROWS - 1) / SEL_ROWS));
  with_ns(c->ns, [&](auto NS) { k_slot_select<decltype(NS)::value><<<grid, 64, 0, c->stream>>>(dst, src, mask_dev, c->B, when); });
  LAUNCHCHK(c);
  return PB_OK;
}
