// abi_recorder.h -- what tests/cpp/estimator_trace.cpp sets on the recording C ABI (tests/cpp/abi_recorder.cpp)
#pragma once

// the kth call from now (1 = the next one) of the C ABI function `fn` logs its line and returns PB_ERR_HIP
void rec_fail_call(const char *fn, int kth);
// what pb_mask_count answers from now on
void rec_set_mask_count(int count);
