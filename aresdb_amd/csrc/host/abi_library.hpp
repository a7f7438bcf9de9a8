// The two libraries behind the cgo C ABI, bound with dlopen:
//   AbiLibrary  <- cgo bindings of query/time_series_aggregate.go:17-19 + cgoutils/memory.go:17-19
//   check       <- the DoCGoCall error convention (cgoutils/utils.go:26-34)
#pragma once

#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "ares_driver.h"
#include "ares_extensions.h"
#include "ares_memory.h"

namespace ares_host {

struct AbiError : std::runtime_error {
  explicit AbiError(const std::string &m) : std::runtime_error(m) {}
};

// DoCGoCall: a non-null pStrErr is the callee's malloc'ed message; the Go host panics with it
inline intptr_t check(CGoCallResHandle h) {
  if (h.pStrErr) {
    std::string msg(h.pStrErr);
    free(const_cast<char *>(h.pStrErr));
    throw AbiError(msg);
  }
  return reinterpret_cast<intptr_t>(h.res);
}

// The extensions' convention (include/ares_extensions.h): a message that starts with the words below is no error, the library
// declines the shape.  true: the message has been freed and the caller latches — the shape does not change, stop asking.
inline bool declined(CGoCallResHandle h) {
  if (!h.pStrErr || strncmp(h.pStrErr, "not fusable", 11) != 0) return false;
  free(const_cast<char *>(h.pStrErr));
  return true;
}

inline void set_err(char *err, int errLen, const char *msg) {
  if (err && errLen > 0) {
    strncpy(err, msg, static_cast<size_t>(errLen) - 1);
    err[errLen - 1] = 0;
  }
}

struct AbiLibrary {
  void *algoHandle = nullptr, *memHandle = nullptr;
  // libalgorithm
  decltype(&::InitIndexVector) InitIndexVector;
  decltype(&::HashLookup) HashLookup;
  decltype(&::UnaryTransform) UnaryTransform;
  decltype(&::UnaryFilter) UnaryFilter;
  decltype(&::BinaryTransform) BinaryTransform;
  decltype(&::BinaryFilter) BinaryFilter;
  decltype(&::Sort) Sort;
  decltype(&::Reduce) Reduce;
  decltype(&::HashReduce) HashReduce;
  decltype(&::AresFusedFilterHashReduce) FusedFilterHashReduce = nullptr;  // optional extension
  decltype(&::AresHintFusedBatch) HintFusedBatch = nullptr;                // optional extension: the batch's plan, said before its filters
  decltype(&::AresScanAtFilterStats) ScanAtFilterStats = nullptr;          // ... and what became of the hints
  decltype(&::AresFusedFilterSelect) FusedFilterSelect = nullptr;          // optional extension
  decltype(&::AresFusedFilterJoinSelect) FusedFilterJoinSelect = nullptr;  // optional extension
  decltype(&::AresJoinColumnsRun) JoinColumnsRun = nullptr;                // optional extension, with ...
  decltype(&::AresJoinColumnBytes) JoinColumnBytes = nullptr;              // ... the size of one of its outputs
  decltype(&::AresGeoShapeColumnRun) GeoShapeColumnRun = nullptr;          // optional extension, with ...
  decltype(&::AresGeoShapeColumnBytes) GeoShapeColumnBytes = nullptr;      // ... the size of its output
  decltype(&::AresLocalTimeColumnRun) LocalTimeColumnRun = nullptr;        // optional extension (sized by JoinColumnBytes)
  decltype(&::Expand) Expand;
  // libmem
  decltype(&::DeviceAllocate) DeviceAllocate;
  decltype(&::DeviceFree) DeviceFree;
  decltype(&::WaitForCudaStream) WaitForCudaStream;
  decltype(&::HyperLogLog) HyperLogLog;
  decltype(&::GeoBatchIntersects) GeoBatchIntersects;
  decltype(&::WriteGeoShapeDim) WriteGeoShapeDim;
  decltype(&::AsyncCopyDeviceToDevice) AsyncCopyDeviceToDevice;
  decltype(&::AsyncCopyDeviceToHost) AsyncCopyDeviceToHost;
  decltype(&::AsyncCopyHostToDevice) AsyncCopyHostToDevice;
  decltype(&::HostAlloc) HostAlloc;
  decltype(&::HostFree) HostFree;
  // optional (include/ares_extensions.h): libmem.so clears a freed block only where something wrote, so
  // whatever writes DeviceAllocate memory behind its back — a collective receiving into it — says so
  void (*NoteWrite)(int, const void *, size_t) = nullptr;
  // ... and whoever submits work to the query's streams behind its back says that too: frees that follow one another with
  // nothing submitted in between share their fence events (a collective is such a submission)
  void (*NoteActivity)() = nullptr;
  void noteWrite(int device, const void *p, size_t bytes) const {
    if (NoteWrite) NoteWrite(device, p, bytes);
    if (NoteActivity) NoteActivity();
  }

  template <typename F>
  void bind(void *handle, const char *name, F &fn, bool optional = false) {
    fn = reinterpret_cast<F>(dlsym(handle, name));
    if (!fn && !optional) throw AbiError(std::string("missing symbol ") + name);
  }

  AbiLibrary(const char *algoPath, const char *memPath) {
    memHandle = dlopen(memPath, RTLD_NOW | RTLD_LOCAL);
    if (!memHandle) throw AbiError(std::string("dlopen ") + memPath + ": " + dlerror());
    algoHandle = dlopen(algoPath, RTLD_NOW | RTLD_LOCAL);
    if (!algoHandle) throw AbiError(std::string("dlopen ") + algoPath + ": " + dlerror());
    bind(algoHandle, "InitIndexVector", InitIndexVector);
    bind(algoHandle, "HashLookup", HashLookup);
    bind(algoHandle, "UnaryTransform", UnaryTransform);
    bind(algoHandle, "UnaryFilter", UnaryFilter);
    bind(algoHandle, "BinaryTransform", BinaryTransform);
    bind(algoHandle, "BinaryFilter", BinaryFilter);
    bind(algoHandle, "Sort", Sort);
    bind(algoHandle, "Reduce", Reduce);
    bind(algoHandle, "HashReduce", HashReduce);
    bind(algoHandle, "HyperLogLog", HyperLogLog);
    bind(algoHandle, "GeoBatchIntersects", GeoBatchIntersects);
    bind(algoHandle, "WriteGeoShapeDim", WriteGeoShapeDim);
    bind(algoHandle, "Expand", Expand);
    bind(algoHandle, "AresFusedFilterHashReduce", FusedFilterHashReduce, true);
    bind(algoHandle, "AresHintFusedBatch", HintFusedBatch, true);
    bind(algoHandle, "AresScanAtFilterStats", ScanAtFilterStats, true);
    bind(algoHandle, "AresFusedFilterSelect", FusedFilterSelect, true);
    bind(algoHandle, "AresFusedFilterJoinSelect", FusedFilterJoinSelect, true);
    bind(algoHandle, "AresJoinColumnsRun", JoinColumnsRun, true);
    bind(algoHandle, "AresJoinColumnBytes", JoinColumnBytes, true);
    bind(algoHandle, "AresGeoShapeColumnRun", GeoShapeColumnRun, true);
    bind(algoHandle, "AresGeoShapeColumnBytes", GeoShapeColumnBytes, true);
    bind(algoHandle, "AresLocalTimeColumnRun", LocalTimeColumnRun, true);
    bind(memHandle, "DeviceAllocate", DeviceAllocate);
    bind(memHandle, "DeviceFree", DeviceFree);
    bind(memHandle, "WaitForCudaStream", WaitForCudaStream);
    bind(memHandle, "AsyncCopyDeviceToDevice", AsyncCopyDeviceToDevice);
    bind(memHandle, "AsyncCopyDeviceToHost", AsyncCopyDeviceToHost);
    bind(memHandle, "AsyncCopyHostToDevice", AsyncCopyHostToDevice);
    bind(memHandle, "HostAlloc", HostAlloc);
    bind(memHandle, "HostFree", HostFree);
    bind(memHandle, "AresMemNoteWrite", NoteWrite, true);
    bind(memHandle, "AresMemNoteActivity", NoteActivity, true);
  }
  ~AbiLibrary() {
    if (algoHandle) dlclose(algoHandle);
    if (memHandle) dlclose(memHandle);
  }
};

// The reference header gives ForeignColumnVector a `*const` member, which makes InputVector neither
// default-constructible nor assignable in C++; a zeroed byte box with the same layout is.
template <typename T>
struct Pod {
  alignas(T) unsigned char bytes[sizeof(T)];
  Pod() { memset(bytes, 0, sizeof(bytes)); }
  T &operator*() { return *reinterpret_cast<T *>(bytes); }
  T *operator->() { return reinterpret_cast<T *>(bytes); }
  const T &get() const { return *reinterpret_cast<const T *>(bytes); }
};
using IV = Pod<InputVector>;
using OV = Pod<OutputVector>;

}  // namespace ares_host
