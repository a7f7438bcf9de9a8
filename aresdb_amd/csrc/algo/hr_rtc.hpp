// Run-time compiled, per-plan specialised scan / merge kernels of the fused HashReduce (hr_rtc.hip; their source: hr_rtc_gen.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <memory>

#include "hr_rtc_gen.hpp"

namespace ares {
namespace hr { struct Workspace; }

// A loaded kernel.  The handle keeps it alive: the cache may drop the entry (least recently used shapes go when it
// is full), the module is unloaded when the last handle is gone.  Null = not available (unsupported shape, no
// hiprtc, does not compile, or still being compiled on a background thread): the caller uses the generic kernel.
struct RtcEntry;
using RtcKernel = std::shared_ptr<RtcEntry>;

// hiprtc could be loaded (and ARES_RTC is not 0)
bool rtc_scan_available();
// workgroups (= private record streams per partition) for a batch of `rows` rows
int rtc_scan_grid(int64_t rows);
// tiles (4096 rows) each workgroup of the compact scan walks — its chunk is contiguous —, or 0 when a chunk would
// not fit the record's row field (chunk rows <= 1 << (partBits + 9)): the caller takes the 16-byte records
int rtc_compact_chunk_tiles(int64_t rows, int partBits);

// The loaded kernel of a shape (rtc_spec_*: comparison and + - x constants are kernel arguments, divisors literals), or
// null.  `wait`: build it on this thread if it is not there yet (otherwise it is built in the background and null is
// returned this time; ARES_RTC_ASYNC=0 makes every lookup wait).
RtcKernel rtc_lookup(int device, const RtcSpec &spec, bool wait = false);

// A plan-sourced scan (`kind`: what the kernel was looked up as) over rows [0, length) of the plan's columns; records
// number their rows from rowBase.  hostCount (RTC_SCAN_COMPACT only): ws.streams words of host memory the device can write
// (the calling thread's pinned slot): every workgroup leaves the number of its rows that passed the filters there.
void rtc_scan_launch(const RtcKernel &kernel, RtcKind kind, const FusedPlanD &plan, uint32_t rowBase, int length, const hr::Workspace &ws,
                     hipStream_t stream, uint32_t *hostCount = nullptr);
// A vector-sourced scan (RTC_VECTOR_SCAN, RTC_SORT_VECTOR_SCAN, RTC_HLL_SCAN) over rows [rowBase, rowBase + length) of a
// materialised dimension vector (widths: as the spec's, null = all four bytes) and the `length` measures at `measures`.
// totalPartBits / spread: Sort + Reduce's level-1 partition (rtc_spec_sort_vector_scan).
void rtc_vector_scan_launch(const RtcKernel &kernel, RtcKind kind, const uint8_t *dimValues, size_t capacity, const void *measures, int nd,
                            const int *widths, uint32_t rowBase, int length, const hr::Workspace &ws, hipStream_t stream,
                            int totalPartBits = 0, bool spread = false);
struct RtcImageArgs {  // device pointers: images of hr::kSlots x 16 bytes per partition, one group count per partition
  const void *in;
  void *out;
  const uint32_t *inCount;
  uint32_t *outCount;
  uint32_t knownOut;  // leading rows of the output dimension vector that already hold the query's groups (image == 2)
};
// hostOut: four words of host memory the device can write (the calling thread's pinned slot): the kernel's last workgroup
// leaves ws.outCount[0 .. 3] there, so the caller waits for the stream instead of enqueueing a copy (ws.outCount[4] must be 0)
void rtc_merge_launch(const RtcKernel &kernel, const FusedPlanD &plan, const uint8_t *prevDims, size_t prevCapacity,
                      const uint8_t *prevValues, uint32_t prevSize, uint8_t *dimOut, size_t outCapacity, uint8_t *outValues,
                      const hr::Workspace &ws, hipStream_t stream, const RtcImageArgs *image = nullptr, uint32_t *hostOut = nullptr);

}  // namespace ares
