// abi_recorder.h -- what tests/cpp/estimator_trace.cpp and tests/cpp/handler_trace.cpp set on, and ask of, the recording C ABI
// (tests/cpp/abi_recorder.cpp)
#pragma once
#include <cstddef>
#include <string>

// the kth call from now (1 = the next one) of the C ABI function `fn` logs its line and returns PB_ERR_HIP
void rec_fail_call(const char *fn, int kth);
// what pb_mask_count answers from now on
void rec_set_mask_count(int count);
// the recorder's form of a pointer, for a driver that prints what an update object holds: NULL | host:<FNV-1a of host_bytes> |
// dev#<ordinal>+<offset> (a pb_malloc'ed block, whatever `mem` says) | dev:foreign
std::string rec_ptr(const void *p, int mem, size_t host_bytes);
