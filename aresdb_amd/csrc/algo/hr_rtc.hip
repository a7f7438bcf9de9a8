// The run-time side of the per-plan specialised scan / merge kernels whose source hr_rtc_gen.hip writes: the hiprtc binding,
// the kernel cache with the shape-keyed map in front of it, the on-disk cache of code objects, the build thread, the launches.
// Compilation never sits on a query's critical path: a kernel that is not loaded yet is compiled on a
// background thread (ARES_RTC_ASYNC=0: inline) while the caller goes on with the generic kernels — which
// stay the fallback at every step —, code objects are kept in an on-disk cache keyed on (architecture,
// hiprtc version, source) so that a restarted process loads instead of compiling, and the in-memory cache is
// bounded (least recently used shapes are unloaded).
// hiprtc is loaded with dlopen: a host without it simply keeps the generic kernel.  ARES_RTC=0: off.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <cerrno>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <fstream>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "hash_reduce_lds.hpp"
#include "hr_kernels.hpp"
#include "hr_rtc.hpp"

namespace ares {

bool phases_enabled() {
  static const bool on = [] { const char *e = getenv("ARES_HR_PHASES"); return e && e[0] == '1'; }();
  return on;
}

namespace {

// ---- the minimum of the hiprtc API, resolved at run time ---------------------------------------------
typedef struct _hiprtcProgram *RtcProgram;
struct RtcApi {
  int (*create)(RtcProgram *, const char *, const char *, int, const char **, const char **) = nullptr;
  int (*compile)(RtcProgram, int, const char **) = nullptr;
  int (*logSize)(RtcProgram, size_t *) = nullptr;
  int (*log)(RtcProgram, char *) = nullptr;
  int (*codeSize)(RtcProgram, size_t *) = nullptr;
  int (*code)(RtcProgram, char *) = nullptr;
  int (*destroy)(RtcProgram *) = nullptr;
  int (*version)(int *, int *) = nullptr;
  bool ok = false;
};
const RtcApi &rtc_api() {
  static const RtcApi api = [] {
    RtcApi a;
    const char *e = getenv("ARES_RTC");
    if (e && e[0] == '0') return a;
    void *h = dlopen("libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("libhiprtc.so.7", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return a;
    a.create = reinterpret_cast<decltype(a.create)>(dlsym(h, "hiprtcCreateProgram"));
    a.compile = reinterpret_cast<decltype(a.compile)>(dlsym(h, "hiprtcCompileProgram"));
    a.logSize = reinterpret_cast<decltype(a.logSize)>(dlsym(h, "hiprtcGetProgramLogSize"));
    a.log = reinterpret_cast<decltype(a.log)>(dlsym(h, "hiprtcGetProgramLog"));
    a.codeSize = reinterpret_cast<decltype(a.codeSize)>(dlsym(h, "hiprtcGetCodeSize"));
    a.code = reinterpret_cast<decltype(a.code)>(dlsym(h, "hiprtcGetCode"));
    a.destroy = reinterpret_cast<decltype(a.destroy)>(dlsym(h, "hiprtcDestroyProgram"));
    a.version = reinterpret_cast<decltype(a.version)>(dlsym(h, "hiprtcVersion"));
    a.ok = a.create && a.compile && a.logSize && a.log && a.codeSize && a.code && a.destroy;
    return a;
  }();
  return api;
}

struct RtcArgs {  // mirrors `struct Args` of the generated source (args_text, hr_rtc_gen.hip): pointers, 8-byte, then 4-byte fields
  const uint32_t *vals[kFusedCols];
  const uint8_t *nulls[kFusedCols];
  uint32_t *recB;
  uint32_t *countsB;
  uint32_t *overflow;
  uint64_t *phases;
  uint32_t *hostCount;  // compact scan: one survivor count per workgroup, in host memory the device can write (null: none)
  uint4 *recA;
  uint32_t *cursorsA;
  uint64_t capA;
  uint32_t bitOff[kFusedCols];
  uint32_t rowBase;
  int length;
  uint32_t capB;
  uint32_t chunkTiles;
  uint32_t k[kNumConsts];
  uint32_t pad;
};
static_assert(sizeof(RtcArgs) % 8 == 0, "Args is passed as one buffer");

struct RtcMergeArgs {  // mirrors `struct MArgs` of the generated source (generate_merge, hr_rtc_gen.hip)
  const uint32_t *vals[kFusedCols];
  const uint8_t *nulls[kFusedCols];
  const uint32_t *recB;
  const uint32_t *countsB;
  const uint32_t *prevRanges;
  const uint8_t *prevDims;
  const uint8_t *prevValues;
  uint8_t *dimOut;
  uint8_t *outValues;
  uint32_t *outCount;
  uint32_t *outRanges;
  uint64_t prevCapacity, outCapacity;
  uint32_t bitOff[kFusedCols];
  uint32_t capB, streams, prevSize, chunkRows;
  uint64_t *phases;  // ARES_HR_PHASES=1: per-partition time stamps (diagnostics)
  uint32_t k[kNumConsts];
  uint32_t pad;
  const uint4 *recA;  // region A (read by kernels generated with `regionA` only)
  const uint32_t *cursorsA;
  uint64_t capA;
  // table images (kernels generated with `image`): kSlots uint4 per partition = [keys u32 x kSlots][positions u32 x kSlots]
  // [values u64 x kSlots]; one group count per partition; knownOut: leading rows of the output dimension vector that already
  // hold the query's groups
  const uint4 *imgIn;
  uint4 *imgOut;
  const uint32_t *imgInCount;
  uint32_t *imgOutCount;
  uint32_t *hostOut;  // the calling thread's mapped pinned slot (null: the host copies outCount back)
  uint32_t knownOut, pad2;
};
static_assert(sizeof(RtcMergeArgs) % 8 == 0, "MArgs is passed as one buffer");

// ---- kernel cache ------------------------------------------------------------------------------------
}  // namespace

struct RtcEntry {
  int device = 0;
  std::mutex m;
  std::condition_variable cv;
  bool ready = false;      // final: the module is loaded, or there is no kernel (fn == nullptr: generic path)
  bool codeReady = false;  // the code object is here (read from disk / compiled), a query thread has yet to load it
  bool fromDisk = false;
  std::vector<char> code;
  std::string diskPath;
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr;  // nullptr once ready = the source does not compile / load: generic kernel
  std::atomic<uint64_t> lastUse{0};
  ~RtcEntry();
};

// Modules of evicted kernels.  Dropped from the cache and by every caller, a launch may still be executing — the module
// cannot be unloaded on the spot without synchronising the device, which would stall every query on it (round-3 review).
// They wait here instead (a code object is tens of kilobytes); only when a hundred have piled up are the older half
// unloaded behind ONE device synchronisation.
namespace {
std::mutex g_graveMutex;
std::vector<std::pair<int, hipModule_t>> g_graveyard;
constexpr size_t kGraveyardLimit = 128;
}  // namespace

RtcEntry::~RtcEntry() {
  if (!module) return;
  std::vector<std::pair<int, hipModule_t>> unload;
  {
    std::lock_guard<std::mutex> lock(g_graveMutex);
    g_graveyard.emplace_back(device, module);
    if (g_graveyard.size() >= kGraveyardLimit) {
      unload.assign(g_graveyard.begin(), g_graveyard.begin() + kGraveyardLimit / 2);
      g_graveyard.erase(g_graveyard.begin(), g_graveyard.begin() + kGraveyardLimit / 2);
    }
  }
  if (unload.empty()) return;
  int current = 0;
  const bool have = hipGetDevice(&current) == hipSuccess;
  int synced = -1;
  for (auto &dm : unload) {
    if (dm.first != synced) {
      (void)hipSetDevice(dm.first);
      (void)hipDeviceSynchronize();
      synced = dm.first;
    }
    (void)hipModuleUnload(dm.second);
  }
  if (have) (void)hipSetDevice(current);
  (void)hipGetLastError();
}

namespace {

struct RtcCache {
  std::mutex mu;
  std::unordered_map<std::string, std::shared_ptr<RtcEntry>> map;  // device + entry point + source -> kernel
  std::mutex frontMu;
  std::unordered_map<std::string, RtcKernel> front;  // spec + device -> loaded kernel (rtc_lookup)
  std::atomic<uint64_t> tick{0};
  std::atomic<int> pending{0};
  std::mutex idleMu;
  std::condition_variable idleCv;
  std::atomic<long> compiles{0}, diskHits{0}, evictions{0};
};
RtcCache &cache() {
  static RtcCache *c = new RtcCache;  // never destroyed: its modules must not outlive the HIP runtime's teardown order
  return *c;
}

size_t cache_capacity() {
  static const size_t cap = [] {
    const char *e = getenv("ARES_RTC_CACHE_ENTRIES");
    const long v = e ? atol(e) : 256;
    return static_cast<size_t>(v < 4 ? 4 : v);
  }();
  return cap;
}

bool rtc_async() {
  static const bool on = [] {
    const char *e = getenv("ARES_RTC_ASYNC");
    return !(e && e[0] == '0');
  }();
  return on;
}

// on-disk cache of code objects: ARES_RTC_CACHE_DIR, else $XDG_CACHE_HOME/aresdb_amd/rtc, else ~/.cache/aresdb_amd/rtc;
// "0" / "off" / "" switches it off
std::string disk_dir() {
  static const std::string dir = [] {
    std::string d;
    if (const char *e = getenv("ARES_RTC_CACHE_DIR")) {
      d = e;
      if (d == "0" || d == "off") d.clear();
      if (d.empty()) return d;
    } else if (const char *x = getenv("XDG_CACHE_HOME")) {
      d = std::string(x) + "/aresdb_amd/rtc";
    } else if (const char *h = getenv("HOME")) {
      d = std::string(h) + "/.cache/aresdb_amd/rtc";
    } else {
      return d;
    }
    std::string partial;  // mkdir -p
    for (size_t i = 0; i <= d.size(); i++)
      if (i == d.size() || (d[i] == '/' && i > 0)) {
        partial = d.substr(0, i);
        if (mkdir(partial.c_str(), 0700) != 0 && errno != EEXIST) return std::string();
      }
    return d;
  }();
  return dir;
}

constexpr uint64_t kDiskMagic = 0x3143545253455241ull;  // "ARESRTC1"
uint64_t fnv1a(const std::string &s, uint64_t h) {
  for (unsigned char c : s) {
    h ^= c;
    h *= 1099511628211ull;
  }
  return h;
}

// the options every kernel is compiled with (part of the on-disk cache key: a change here must not load old code)
constexpr const char *kRtcOptions[] = {"-O3", "-std=c++17", "-munsafe-fp-atomics"};
constexpr int kRtcOptionCount = 3;

std::string disk_name(const std::string &arch, const std::string &source) {
  int major = 0, minor = 0, runtime = 0;
  if (rtc_api().version) (void)rtc_api().version(&major, &minor);
  if (hipRuntimeGetVersion(&runtime) != hipSuccess) {  // carries the patch level the hiprtc pair lacks
    (void)hipGetLastError();
    runtime = 0;
  }
  std::string salt = arch + "|hiprtc " + std::to_string(major) + "." + std::to_string(minor) + "|runtime " + std::to_string(runtime) + "|";
  for (int k = 0; k < kRtcOptionCount; k++) salt += std::string(kRtcOptions[k]) + " ";
  salt += "|";
  char b[48];
  snprintf(b, sizeof(b), "%016llx%016llx.co", static_cast<unsigned long long>(fnv1a(source, fnv1a(salt, 14695981039346656037ull))),
           static_cast<unsigned long long>(fnv1a(source, fnv1a(salt, 0x9e3779b97f4a7c15ull))));
  return b;
}

std::string device_arch(int device) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
    (void)hipGetLastError();
    return "gfx950";
  }
  return prop.gcnArchName[0] ? std::string(prop.gcnArchName) : std::string("gfx950");
}

bool compile_source(const std::string &source, const std::string &arch, const char *entry, std::vector<char> &code) {
  const RtcApi &api = rtc_api();
  RtcProgram prog = nullptr;
  if (!api.ok || !api.create) return false;  // (no hiprtc in this process: callers check rtc_scan_available() first)
  if (api.create(&prog, source.c_str(), "hr_rtc.hip", 0, nullptr, nullptr) != 0) return false;
  const std::string archOpt = "--offload-arch=" + arch;
  const char *opts[1 + kRtcOptionCount] = {archOpt.c_str()};
  for (int k = 0; k < kRtcOptionCount; k++) opts[1 + k] = kRtcOptions[k];
  bool ok = false;
  if (api.compile(prog, 1 + kRtcOptionCount, opts) == 0) {
    size_t size = 0;
    if (api.codeSize(prog, &size) == 0 && size) {
      code.resize(size);
      ok = api.code(prog, code.data()) == 0;
    }
  } else {
    size_t n = 0;
    std::string log;
    if (api.logSize(prog, &n) == 0 && n) {
      log.resize(n);
      api.log(prog, &log[0]);
    }
    fprintf(stderr, "libalgorithm: hiprtc could not compile %s (generic kernel used): %s\n", entry, log.c_str());
  }
  api.destroy(&prog);
  return ok;
}

// ARES_RTC_TRACE=<file>: one line per kernel build — where its time went (diagnostics of cold starts)
void rtc_trace(const char *what, const std::string &entry, double ms, size_t bytes) {
  static const char *path = getenv("ARES_RTC_TRACE");
  if (!path || !path[0]) return;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if (FILE *o = fopen(path, "a")) {
    const double now = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
    fprintf(o, "%.3f %s %s %.3f ms %zu bytes\n", now, what, entry.c_str(), ms, bytes);
    fclose(o);
  }
}
struct TraceClock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// ---- building an entry -----------------------------------------------------------------------------------------
// A code object comes from the on-disk cache (read by the CALLER: tens of microseconds) or from hiprtc (seconds: on a
// background thread unless ARES_RTC_ASYNC=0 / `wait`).  hipModuleLoadData ALWAYS runs on a calling (query) thread, the
// first one that finds the code ready: 0.2-0.7 ms there.  On a background thread the same load was once seen to take
// 530 ms — queued behind a 4.3 GB hipMalloc of the query thread (the runtime serialises the two), which is what the
// "490 ms first query of a process that finds its kernels on disk" of round 3 really was: the DIRECT-mode workspace,
// sized for a region that mode does not write (hash_reduce_lds.hip, profiles/r4_experiments.md "cold start").
std::string disk_path(int device, const std::string &source) {
  const std::string dir = disk_dir();
  return dir.empty() ? std::string() : dir + "/" + disk_name(device_arch(device), source);
}

bool read_disk(const std::string &path, const std::string &entryName, std::vector<char> &code) {
  code.clear();
  if (path.empty()) return false;
  TraceClock tRead;
  std::ifstream in(path, std::ios::binary | std::ios::ate);  // file = {magic, code bytes, FNV-1a of the code} + code
  if (!in) return false;
  const std::streamsize n = in.tellg();
  uint64_t head[3] = {0, 0, 0};
  if (n > static_cast<std::streamsize>(sizeof(head))) {
    in.seekg(0);
    if (in.read(reinterpret_cast<char *>(head), sizeof(head)) && head[0] == kDiskMagic && head[1] == static_cast<uint64_t>(n) - sizeof(head)) {
      code.resize(static_cast<size_t>(head[1]));
      if (!in.read(code.data(), static_cast<std::streamsize>(code.size())) ||
          fnv1a(std::string(code.data(), code.size()), 14695981039346656037ull) != head[2])
        code.clear();
    }
  }
  if (code.empty()) {
    (void)unlink(path.c_str());  // truncated, corrupted or of another format
    return false;
  }
  rtc_trace("disk_read", entryName, tRead.ms(), code.size());
  return true;
}

void write_disk(const std::string &path, const std::vector<char> &code) {  // publish atomically: write aside, then rename
  if (path.empty() || code.empty()) return;
  const std::string tmp = path + ".tmp" + std::to_string(static_cast<long>(getpid())) + "." + std::to_string(cache().tick.load());
  std::ofstream out(tmp, std::ios::binary);
  const uint64_t head[3] = {kDiskMagic, static_cast<uint64_t>(code.size()), fnv1a(std::string(code.data(), code.size()), 14695981039346656037ull)};
  if (out && out.write(reinterpret_cast<const char *>(head), sizeof(head)) && out.write(code.data(), static_cast<std::streamsize>(code.size())) &&
      (out.close(), true)) {
    if (rename(tmp.c_str(), path.c_str()) != 0) (void)unlink(tmp.c_str());
  } else {
    (void)unlink(tmp.c_str());
  }
}

// caller holds e->m and has selected e->device: the entry's code becomes its kernel (or "no kernel": generic path)
void load_entry(RtcEntry &e, const std::string &entryName) {
  TraceClock tLoad;
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr;
  if (!e.code.empty() && hipModuleLoadData(&module, e.code.data()) == hipSuccess) {
    if (hipModuleGetFunction(&fn, module, entryName.c_str()) != hipSuccess) fn = nullptr;
  } else {
    module = nullptr;
  }
  (void)hipGetLastError();
  rtc_trace("module_load", entryName, tLoad.ms(), e.code.size());
  if (fn) {  // (a kernel with scratch memory pays a queue-wide scratch allocation at its first launch)
    int scratch = 0;
    if (hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, fn) == hipSuccess)
      rtc_trace("scratch_bytes_per_lane", entryName, 0.0, static_cast<size_t>(scratch));
    (void)hipGetLastError();
  }
  if (!fn && e.fromDisk && !e.diskPath.empty()) (void)unlink(e.diskPath.c_str());  // a stale cache file
  if (fn && !e.fromDisk) write_disk(e.diskPath, e.code);
  e.code.clear();
  e.code.shrink_to_fit();
  e.module = module;
  e.fn = fn;
  e.codeReady = false;
  e.ready = true;
}

// hiprtc on this thread (the caller's, or a background thread): leaves the code in the entry for a query thread to load
void compile_entry(const std::shared_ptr<RtcEntry> &e, const std::string &source, const std::string &entryName) {
  RtcCache &c = cache();
  std::vector<char> code;
  TraceClock tCompile;
  const bool ok = compile_source(source, device_arch(e->device), entryName.c_str(), code);
  c.compiles++;
  rtc_trace("hiprtc_compile", entryName, tCompile.ms(), code.size());
  {
    std::lock_guard<std::mutex> lock(e->m);
    if (ok) {
      e->code.swap(code);
      e->codeReady = true;
    } else {
      e->ready = true;  // no kernel: the generic path
    }
  }
  e->cv.notify_all();
  if (c.pending.fetch_sub(1) == 1) {
    std::lock_guard<std::mutex> lock(c.idleMu);
    c.idleCv.notify_all();
  }
}

void wait_idle() {
  RtcCache &c = cache();
  std::unique_lock<std::mutex> lock(c.idleMu);
  c.idleCv.wait(lock, [&] { return c.pending.load() == 0; });
}

// The kernel of this source on `device`: the loaded kernel, or null while it is being built on a background
// thread (the caller uses the generic kernel this time), or — `wait` / ARES_RTC_ASYNC=0 — after building it.
RtcKernel compiled_kernel(int device, const std::string &source, const char *entry, bool wait) {
  if (source.empty()) return nullptr;
  RtcCache &c = cache();
  const std::string key = std::to_string(device) + "|" + entry + "|" + source;
  std::shared_ptr<RtcEntry> e;
  std::vector<std::shared_ptr<RtcEntry>> evicted;  // destroyed (device synchronised, module unloaded) outside the lock
  bool created = false;
  {
    std::lock_guard<std::mutex> lock(c.mu);
    auto it = c.map.find(key);
    if (it != c.map.end()) {
      e = it->second;
    } else {
      while (c.map.size() >= cache_capacity()) {  // drop the least recently used kernel that is not being built
        auto victim = c.map.end();
        for (auto jt = c.map.begin(); jt != c.map.end(); ++jt) {
          bool ready;
          {  // (an entry whose code is here but that nobody asked for again has no module yet: dropping it is free)
            std::lock_guard<std::mutex> el(jt->second->m);
            ready = jt->second->ready || jt->second->codeReady;
          }
          if (ready && (victim == c.map.end() || jt->second->lastUse.load() < victim->second->lastUse.load())) victim = jt;
        }
        if (victim == c.map.end()) break;
        evicted.push_back(victim->second);
        c.map.erase(victim);
        c.evictions++;
      }
      e = std::make_shared<RtcEntry>();
      e->device = device;
      c.map.emplace(key, e);
      created = true;
      c.pending++;
      static const int registered = atexit([] { wait_idle(); });  // no build thread outlives the process's exit handlers
      (void)registered;
    }
    e->lastUse.store(++c.tick);
  }
  evicted.clear();
  if (created) {
    e->diskPath = disk_path(device, source);
    std::vector<char> code;
    if (read_disk(e->diskPath, entry, code)) {  // found on disk: loaded below, on this thread
      c.diskHits++;
      {
        std::lock_guard<std::mutex> lock(e->m);
        e->code.swap(code);
        e->fromDisk = true;
        e->codeReady = true;
      }
      e->cv.notify_all();  // (a second thread may already wait for this entry: `wait` / ARES_RTC_ASYNC=0)
      if (c.pending.fetch_sub(1) == 1) {
        std::lock_guard<std::mutex> idle(c.idleMu);
        c.idleCv.notify_all();
      }
    } else if (rtc_async() && !wait) {
      std::thread([e, source, name = std::string(entry)] { compile_entry(e, source, name); }).detach();
    } else {
      compile_entry(e, source, entry);
    }
  }
  std::unique_lock<std::mutex> lock(e->m);
  if (!e->ready && !e->codeReady) {
    if (rtc_async() && !wait) return nullptr;
    e->cv.wait(lock, [&] { return e->ready || e->codeReady; });
  }
  if (!e->ready) {  // the code is here: this (query) thread loads it
    (void)hipSetDevice(device);
    load_entry(*e, entry);
    e->cv.notify_all();
  }
  return e->fn ? e : nullptr;
}

// what of a plan is run-time arguments of both kernels: the column slots and the dimensions' constants
template <typename Args>
void fill_columns(Args &args, const FusedPlanD &plan) {
  memset(&args, 0, sizeof(args));
  for (int c = 0; c < plan.numCols; c++) {
    args.vals[c] = plan.cols[c].vals;
    args.nulls[c] = plan.cols[c].nulls;
    args.bitOff[c] = plan.cols[c].bitOff;
  }
  for (int d = 0; d < kFusedDims; d++) {
    args.k[const_slot_dim(d)] = plan.dims[d].f.bbits;
    for (int k = 0; k < plan.dims[d].f.chain.n && k < kMaxChainSteps; k++) args.k[const_slot_dim_chain(d) + k] = plan.dims[d].f.chain.s[k].bbits;
  }
  for (int k = 0; k < plan.measure.f.chain.n && k < kMaxChainSteps; k++) args.k[const_slot_measure_chain() + k] = plan.measure.f.chain.s[k].bbits;
}

// ARES_HR_PHASES=1 (diagnostics): a kernel family's device buffer of 8 time stamps per workgroup, and its launch count
struct PhaseReport {
  uint64_t *dev = nullptr;
  int launches = 0;
  uint64_t *buffer(size_t workgroups) {
    if (!dev) hip_check(hipMalloc(reinterpret_cast<void **>(&dev), sizeof(uint64_t) * 8 * workgroups), "hipMalloc");
    return dev;
  }
  // the stamps of `workgroups` workgroups once the stream has run; true: this launch is one to report (the first three, then
  // every 64th)
  bool fetch(std::vector<uint64_t> &h, int workgroups, hipStream_t stream) {
    h.resize(static_cast<size_t>(8) * workgroups);
    hip_check(hipMemcpyAsync(h.data(), dev, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    return ++launches <= 3 || launches % 64 == 0;
  }
};

void launch(const RtcKernel &kernel, void *args, size_t size, unsigned grid, hipStream_t stream, const char *name) {
  void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  KernelTimer timer(name, stream);
  hip_check(hipModuleLaunchKernel(kernel->fn, grid, 1, 1, hr::kThreads, 1, 1, 0, stream, nullptr, config), "hipModuleLaunchKernel");
}

// `plan`: the columns and constants of a scan (RtcArgs::k: comparison constants converted to the common kind by the host)
void launch_scan(const RtcKernel &kernel, const FusedPlanD &plan, uint32_t rowBase, int length, const hr::Workspace &ws, int grid,
                 uint32_t chunkTiles, uint32_t pad, hipStream_t stream, const char *name, uint32_t *hostCount = nullptr) {
  RtcArgs args;
  fill_columns(args, plan);
  for (int k = 0; k < plan.numFilters && k < kFusedFilters; k++)
    args.k[const_slot_filter(k)] = host_cvt32(plan.filters[k].f.bbits, plan.filters[k].f.bkind, plan.filters[k].f.I);
  args.k[const_slot_measure()] = plan.measure.f.bbits;
  args.recB = ws.recB;
  args.countsB = ws.countsB;
  args.overflow = ws.outCount + 1;
  args.hostCount = hostCount;
  args.recA = ws.recA;
  args.cursorsA = ws.cursorsA;
  args.capA = ws.capA;
  args.rowBase = rowBase;
  args.length = length;
  args.capB = ws.capB;
  args.chunkTiles = chunkTiles;
  args.pad = pad;
  static PhaseReport report;
  if (phases_enabled()) args.phases = report.buffer(hr::kMaxStreams);
  launch(kernel, &args, sizeof(args), static_cast<unsigned>(grid), stream, name);
  std::vector<uint64_t> h;
  if (phases_enabled() && report.fetch(h, grid, stream)) {  // core-clock cycles lane 0 of each workgroup spent per phase
    double sum[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int g = 0; g < grid; g++)
      for (int k = 0; k < 7; k++) sum[k] += static_cast<double>(h[static_cast<size_t>(8) * g + k]);
    const double n = grid * 1e3;
    fprintf(stderr, "%s phases (launch %d, %d workgroups, %d rows): kcycles per workgroup: eval+count %.1f, scan %.1f, scatter %.1f, lines %.1f, leftovers %.1f, drain %.1f, last lines %.1f\n",
            name, report.launches, grid, length, sum[0] / n, sum[1] / n, sum[2] / n, sum[3] / n, sum[4] / n, sum[5] / n, sum[6] / n);
  }
}

}  // namespace

bool rtc_scan_available() { return rtc_api().ok; }

// number of workgroups (= private streams per partition) the specialised kernels want for `rows` rows: one per tile up to
// hr::kMaxStreams.  Forcing several tiles per workgroup on small batches (fewer, longer runs for the merge) lengthened the
// scan by more than it saved in the merge (profiles/r5_experiments.md).
int rtc_scan_grid(int64_t rows) {
  const int64_t tiles = (rows + 4095) / 4096;
  return static_cast<int>(tiles < hr::kMaxStreams ? (tiles < 1 ? 1 : tiles) : hr::kMaxStreams);
}

// tiles per workgroup of the compact scan, 0 when a chunk would not fit the record's row field
int rtc_compact_chunk_tiles(int64_t rows, int partBits) {
  if (partBits < 3 || rows <= 0) return 0;
  const int64_t tiles = (rows + 4095) / 4096;
  const int64_t grid = rtc_scan_grid(rows);
  const int64_t chunk = (tiles + grid - 1) / grid;
  return chunk <= (1ll << (partBits - 3)) ? static_cast<int>(chunk) : 0;
}

// ---- lookup by shape, without writing the source -----------------------------------------------------------
// The kernel cache is keyed by source text; writing a kernel's text (tens of kilobytes through a string stream) and
// comparing it costs tens of microseconds — twice per HashReduce call, 30 times per 1 B-row query, a third of a
// 2 Mi-row live batch's host time.  In front of it: a small map from the spec's bytes (all the generators read) and
// the device to the loaded kernel.  Only loaded kernels are entered; a miss takes the long way and is always right.
RtcKernel rtc_lookup(int device, const RtcSpec &spec, bool wait) {
  if (!rtc_api().ok) return nullptr;
  std::string key(reinterpret_cast<const char *>(&spec), sizeof(spec));
  key.append(reinterpret_cast<const char *>(&device), sizeof(device));
  RtcCache &c = cache();
  {
    std::lock_guard<std::mutex> lock(c.frontMu);
    auto it = c.front.find(key);
    if (it != c.front.end()) return it->second;
  }
  RtcKernel k = compiled_kernel(device, rtc_source(spec), rtc_entry_name(spec.kind), wait);
  if (k) {
    std::lock_guard<std::mutex> lock(c.frontMu);
    if (c.front.size() >= 64) c.front.clear();  // holds references: bounded well below the main cache's capacity
    c.front.emplace(key, k);
  }
  return k;
}

void rtc_scan_launch(const RtcKernel &kernel, RtcKind kind, const FusedPlanD &plan, uint32_t rowBase, int length, const hr::Workspace &ws,
                     hipStream_t stream, uint32_t *hostCount) {
  // (TABLE: one workgroup per tile up to a full device — its records do not grow with it)
  const int grid = kind == RTC_SCAN_TABLE ? rtc_scan_grid(length) : ws.streams;
  const uint32_t chunkTiles = kind == RTC_SCAN_COMPACT ? ws.chunkRows / 4096u : 0u;
  launch_scan(kernel, plan, rowBase, length, ws, grid, chunkTiles, 0u, stream,
              kind == RTC_SCAN_TABLE ? "hr_table_scan_rtc" : rtc_entry_name(kind), kind == RTC_SCAN_COMPACT ? hostCount : nullptr);
}

void rtc_vector_scan_launch(const RtcKernel &kernel, RtcKind kind, const uint8_t *dimValues, size_t capacity, const void *measures, int nd,
                            const int *widths, uint32_t rowBase, int length, const hr::Workspace &ws, hipStream_t stream, int totalPartBits,
                            bool spread) {
  FusedPlanD plan;
  memset(&plan, 0, sizeof(plan));
  fused_plan_vector_columns(plan, dimValues, capacity, nd, widths, rowBase);
  plan.cols[nd].vals = static_cast<const uint32_t *>(measures);
  // (Sort + Reduce: the partition expression's shift, and whether it spreads)
  launch_scan(kernel, plan, rowBase, length, ws, ws.streams, totalPartBits > 0 ? static_cast<uint32_t>(32 - totalPartBits) : 0u,
              spread ? 1u : 0u, stream, kind == RTC_SORT_VECTOR_SCAN ? "sr_vector_scan_rtc" : rtc_entry_name(kind));
}

void rtc_merge_launch(const RtcKernel &kernel, const FusedPlanD &plan, const uint8_t *prevDims, size_t prevCapacity, const uint8_t *prevValues,
                      uint32_t prevSize, uint8_t *dimOut, size_t outCapacity, uint8_t *outValues, const hr::Workspace &ws,
                      hipStream_t stream, const RtcImageArgs *image, uint32_t *hostOut) {
  RtcMergeArgs args;
  fill_columns(args, plan);
  args.recB = ws.recB;
  args.countsB = ws.countsB;
  args.prevRanges = ws.prevRanges;
  args.prevDims = prevDims;
  args.prevValues = prevValues;
  args.dimOut = dimOut;
  args.outValues = outValues;
  args.outCount = ws.outCount;
  args.outRanges = ws.outRanges;
  args.prevCapacity = prevCapacity;
  args.outCapacity = outCapacity;
  args.capB = ws.capB;
  args.recA = ws.recA;
  args.cursorsA = ws.cursorsA;
  args.capA = ws.capA;
  args.streams = static_cast<uint32_t>(ws.streams);
  args.prevSize = prevSize;
  args.chunkRows = ws.chunkRows;
  if (image) {
    args.imgIn = reinterpret_cast<const uint4 *>(image->in);
    args.imgOut = reinterpret_cast<uint4 *>(image->out);
    args.imgInCount = image->inCount;
    args.imgOutCount = image->outCount;
    args.knownOut = image->knownOut;
  }
  args.hostOut = hostOut;
  static PhaseReport report;
  if (phases_enabled()) {
    args.phases = report.buffer(hr::kMaxPartitions);
    hip_check(hipMemsetAsync(args.phases, 0, sizeof(uint64_t) * 8 * hr::kMaxPartitions, stream), "hipMemsetAsync");
  }
  launch(kernel, &args, sizeof(args), 1u << ws.partBits, stream, "hr_merge_rtc");
  const int np = 1 << ws.partBits;
  std::vector<uint64_t> h;
  if (phases_enabled() && report.fetch(h, np, stream)) {  // where a partition's time goes (100 MHz constant clock)
    uint64_t first = ~0ull, last = 0;
    double sum[5] = {0, 0, 0, 0, 0}, whole = 0;
    for (int p = 0; p < np; p++) {
      const uint64_t *t = &h[static_cast<size_t>(8) * p];
      if (t[0] < first) first = t[0];
      if (t[5] > last) last = t[5];
      for (int k = 0; k < 5; k++) sum[k] += static_cast<double>(t[k + 1] - t[k]) * 0.01;
      whole += static_cast<double>(t[5] - t[0]) * 0.01;
    }
    fprintf(stderr, "hr_merge_rtc phases (launch %d, %d partitions, prev %u): span %.1f us; per partition avg %.1f us = init %.1f + prev %.1f + records %.1f + count %.1f + emit %.1f\n",
            report.launches, np, prevSize, static_cast<double>(last - first) * 0.01, whole / np, sum[0] / np, sum[1] / np, sum[2] / np, sum[3] / np, sum[4] / np);
  }
}

}  // namespace ares

// Exported (include/ares_extensions.h): blocks until no kernel is being compiled in the background; returns the
// number of kernels the cache holds.  counters (may be null): [0] hiprtc compilations, [1] code objects found in
// the on-disk cache, [2] kernels dropped from the in-memory cache.
extern "C" size_t AresRtcWait(long *counters) {
  ares::wait_idle();
  ares::RtcCache &c = ares::cache();
  if (counters) {
    counters[0] = c.compiles.load();
    counters[1] = c.diskHits.load();
    counters[2] = c.evictions.load();
  }
  std::lock_guard<std::mutex> lock(c.mu);
  return c.map.size();
}
