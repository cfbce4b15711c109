// abi_recorder_wide.cpp -- the recording stand-in for pb_update_indexed_wide, the one C ABI function pronto_amd/csrc/mav_state_est_wide.hpp
// calls beyond those of the two older shim headers.  Linked beside the unchanged tests/cpp/abi_recorder.cpp (which defines the rest and
// stays exactly the list of functions those headers use); one line per call in that recorder's style: name, scalars, the index list in
// full, pointers by kind or checksum, never an address.
#include <cstdio>
#include <string>

#include "../../include/pronto_batch.h"
#include "abi_recorder.h"

// (the recorder's context, as tests/cpp/abi_recorder.cpp defines it: what every update does to the slots is modelled here too)
struct pb_ctx {
  int n, B, nhist = 0;
  int out_slot = -1, pred_slot = -1, head_slot = -1;
  int gets = 0, fills = 0;
};

extern "C" int pb_update_indexed_wide(pb_ctx *c, int m, const int *idx, const double *z, const double *R, int r_kind, const double *quat,
                                      const uint8_t *mask, int mem)
{
  const size_t per = mem == PB_HOST_BROADCAST ? 1 : (size_t) c->B;
  std::string list = "[";
  for (int i = 0; i < m; i++) list += (i ? "," : "") + std::to_string(idx[i]);
  list += "]";
  const std::string cov = r_kind == PB_R_DIAG_BROADCAST ? rec_ptr(R, PB_HOST_BROADCAST, sizeof(double) * m)
                                                        : rec_ptr(R, mem, sizeof(double) * (r_kind == PB_R_FULL ? m * m : m) * per);
  printf("pb_update_indexed_wide m=%d idx=%s z=%s R=%s r_kind=%d quat=%s mask=%s mem=%d\n", m, list.c_str(),
         rec_ptr(z, mem, sizeof(double) * m * per).c_str(), cov.c_str(), r_kind, rec_ptr(quat, mem, sizeof(double) * 4 * per).c_str(),
         rec_ptr(mask, mem, (size_t) c->B).c_str(), mem);
  c->pred_slot = -1;
  c->head_slot = c->out_slot;
  c->out_slot = -1;
  return PB_OK;
}
