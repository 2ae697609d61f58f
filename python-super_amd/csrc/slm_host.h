// slm_host.h -- what every stage host of the library shares: the error channel behind slm_last_error(), the
// num_neighbors dispatch, grow-only device buffers (as a function and as the owning DevBuf / PinnedBuf), rocPRIM scratch
// and the member tables of the stage contexts.
// Host code only (device code includes slm_common.h, never this).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <string>

#include "super_lm.h"

// ---- one error channel: the text slm_last_error() returns (thread-local, slm_api.hip) -------------------------------
void slm_set_error_text(const char* msg);

inline int fail(int code, const char* msg) {
  slm_set_error_text(msg);
  return code;
}
inline int fail(int code, const std::string& msg) { return fail(code, msg.c_str()); }

// a failed HIP call ends the function: with SLM_ERR_HIP and the text "<expr>: <hip error string>" ...
#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) return fail(SLM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
// ... or, in a helper that returns hipError_t itself, with the error
#define HIPRET(expr)                 \
  do {                               \
    hipError_t e_ = (expr);          \
    if (e_ != hipSuccess) return e_; \
  } while (0)

// one instantiation of a per-surfel kernel per opt.num_neighbors: KK = K as a constant for 1..8, nothing otherwise
#define SLM_K_DISPATCH(K, ...)                            \
  switch (K) {                                            \
    case 1: { constexpr int KK = 1; __VA_ARGS__; break; } \
    case 2: { constexpr int KK = 2; __VA_ARGS__; break; } \
    case 3: { constexpr int KK = 3; __VA_ARGS__; break; } \
    case 4: { constexpr int KK = 4; __VA_ARGS__; break; } \
    case 5: { constexpr int KK = 5; __VA_ARGS__; break; } \
    case 6: { constexpr int KK = 6; __VA_ARGS__; break; } \
    case 7: { constexpr int KK = 7; __VA_ARGS__; break; } \
    case 8: { constexpr int KK = 8; __VA_ARGS__; break; } \
    default: break;                                       \
  }

// the KNN-table check of a bind (slm_nodes.hip): *bad (device, zeroed by the caller) = 1 when a surfel's row of sf_knn_idx
// repeats an id or any sf_knn_idx / ed_knn_idx entry lies outside [0, J).  Enqueues one launch on `stream` (a hipStream_t,
// as the C ABI passes it); reads the tables only.
void launch_check_knn(const slm_frame& f, int* bad, void* stream);

// ---- grow-only device buffers ---------------------------------------------------------------------------------------
// A buffer of `cap` elements of `esz` bytes that must hold `need`: nothing to do while need <= cap; otherwise the old
// one is freed and `want` elements are allocated (the caller's head-room rule; need itself for an exact fit).  The
// capacity is 0 from the free until the allocation has succeeded, so it is never non-zero beside a null pointer.
inline hipError_t grow(void*& p, size_t& cap, size_t need, size_t want, size_t esz) {
  if (need <= cap) return hipSuccess;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  HIPRET(hipMalloc(&p, want * esz));
  cap = want;
  return hipSuccess;
}
template <typename T>
hipError_t grow(T*& p, size_t& cap, size_t need, size_t want) {
  void* q = p;
  const hipError_t e = grow(q, cap, need, want, sizeof(T));
  p = static_cast<T*>(q);
  return e;
}

// The same buffer as an owner: move-only, freed by its destructor.  A struct of these (a slot of the LM solver) needs no
// release list, and a descriptor only mirrors `p`.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t grow(size_t need, size_t want) { return ::grow(p, cap, need, want); }
  operator T*() const { return p; }
};

// Host buffer for per-frame device -> host read-backs, PINNED (hipHostMalloc, grow-only), owned like a DevBuf.  A
// read-back into pageable memory (a std::vector) goes through the runtime's staging path, and several bind workers doing
// that at once were seen to block for 5-7 ms together once in ~50 steps (tools/studies/stall_hunt.py: the whole rare
// stall of a bench step sat in this one hipMemcpyAsync + hipStreamSynchronize); a pinned destination is a plain DMA.
template <typename T>
struct PinnedBuf {
  T* p = nullptr;
  size_t cap = 0, n = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap), n(o.n) { o.p = nullptr; o.cap = o.n = 0; }
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  hipError_t grow(size_t need, size_t want) {
    if (need <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = n = 0;
    HIPRET(hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault));
    cap = want;
    return hipSuccess;
  }
  hipError_t resize(size_t need) {   // a read-back of `need` elements, with head-room
    HIPRET(grow(need, need + need / 8 + 16));
    n = need;
    return hipSuccess;
  }
  T* data() { return p; }
  const T* data() const { return p; }
  size_t size() const { return n; }
  T* begin() { return p; }
  T* end() { return p + n; }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
};

// rocPRIM temporary storage (bytes, grow-only, exact): call(nullptr, bytes) reports the size, call(tmp, bytes) runs
template <typename Call>
hipError_t with_scratch(void*& tmp, size_t& cap, Call call) {
  size_t bytes = 0;
  HIPRET(call(nullptr, bytes));
  HIPRET(grow(tmp, cap, bytes, bytes, 1));
  return call(tmp, bytes);
}

// ---- what a stage context owns --------------------------------------------------------------------------------------
// One row per device array of a context struct: where its pointer sits, its element size, and how many elements its
// create function allocates: `mult` times the struct's size number `unit` (0: none, the array grows on demand).
// Allocation (alloc_members) and release (free_members) both walk the table, so what is allocated is also freed.
struct DevMember { size_t ptr, esz, mult; int unit; };
#define DEV_MEMBER(S, name, mult, unit) {offsetof(S, name), sizeof(*((S*)nullptr)->name), mult, unit}
#define DEV_GROWN(S, name) {offsetof(S, name), 0, 0, 0}

template <size_t M>
hipError_t alloc_members(void* s, const DevMember (&tab)[M], const size_t* units) {
  for (const DevMember& a : tab)
    if (a.mult) HIPRET(hipMalloc(reinterpret_cast<void**>((char*)s + a.ptr), a.esz * a.mult * units[a.unit]));
  return hipSuccess;
}
template <size_t M>
void free_members(void* s, const DevMember (&tab)[M]) {
  for (const DevMember& a : tab)
    if (void* q = *reinterpret_cast<void**>((char*)s + a.ptr)) (void)hipFree(q);
}
