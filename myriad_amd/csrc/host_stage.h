// host_stage.h -- Stage: the arrays of one C-ABI call, carved out of one growing device buffer.
//
// The caller registers its arrays in order -- in / out / inout / scratch, each naming the typed device-pointer variable to fill --, then
//   commit(): sizes the buffer (every carve 16-byte aligned, by bytes), grows it once, fills the variables, uploads in registration order;
//   finish(): downloads in registration order and synchronises.
// A host caller (MYR_MEM_HOST) gets every array staged.  A device caller (MYR_MEM_DEVICE) gets its own pointers handed through: only the scratch
// items are reserved, nothing is copied and finish() does nothing (device calls return without a synchronise).  An array the caller did not pass
// (null) or of zero elements gets a null device pointer and no room; out(..., always = true) is the exception a solver needs: the device array
// exists whether or not the host caller asked for the result, and is downloaded only when asked.
//
// Backend: int grow(size_t bytes, void** base), int upload(void* dev, const void* host, size_t bytes), int download(void* host, const void* dev,
// size_t bytes), int sync() -- 0 or the library's error code, which commit() / finish() return as it is.  The library's backend is the HIP runtime on
// the handle's stream; tests/hostsim/stage_check.cpp runs this file on malloc / memcpy under the host sanitizers.  No HIP in here.
#pragma once
#include <assert.h>
#include <stddef.h>

namespace myriad {

template <class Backend>
class Stage {
 public:
  static constexpr int MAX_ITEMS = 24;      // (the restoration working set registers 21)
  Stage(const Backend& be, bool host) : be_(be), host_(host) {}

  template <class T> void in(const T*& dev, const T* user, size_t count) { add<const T>(dev, user, count, UP); }
  template <class T> void out(T*& dev, T* user, size_t count, bool always = false) { add<T>(dev, user, count, always ? DOWN | ALWAYS : DOWN); }
  template <class T> void inout(T*& dev, T* user, size_t count) { add<T>(dev, user, count, UP | DOWN); }
  template <class T> void scratch(T*& dev, size_t count) { add<T>(dev, nullptr, count, SCRATCH); }

  int commit() {
    size_t need = 0;
    for (int i = 0; i < n_; ++i) {
      Item& it = items_[i];
      it.staged = it.bytes > 0 && ((it.kind & SCRATCH) || (host_ && (it.user || (it.kind & ALWAYS))));
      it.off = need;
      if (it.staged) need += (it.bytes + 15) & ~(size_t)15;
    }
    void* base = nullptr;
    if (need)
      if (int rc = be_.grow(need, &base)) return rc;
    for (int i = 0; i < n_; ++i) {
      Item& it = items_[i];
      it.dev = it.staged ? (char*)base + it.off : (host_ || !it.bytes ? nullptr : const_cast<void*>(it.user));
      it.set(it.var, it.dev);
    }
    for (int i = 0; i < n_; ++i)
      if (items_[i].staged && (items_[i].kind & UP))
        if (int rc = be_.upload(items_[i].dev, items_[i].user, items_[i].bytes)) return rc;
    return 0;
  }

  int finish() {
    if (!host_) return 0;
    for (int i = 0; i < n_; ++i)
      if (items_[i].staged && (items_[i].kind & DOWN) && items_[i].user)
        if (int rc = be_.download(const_cast<void*>(items_[i].user), items_[i].dev, items_[i].bytes)) return rc;
    return be_.sync();
  }

  // what commit() laid out (tests)
  int count() const { return n_; }
  bool staged(int i) const { return items_[i].staged; }
  void* device(int i) const { return items_[i].dev; }
  size_t bytes(int i) const { return items_[i].bytes; }

 private:
  enum { UP = 1, DOWN = 2, SCRATCH = 4, ALWAYS = 8 };
  struct Item {
    void* var; void (*set)(void* var, void* p);      // the caller's pointer variable and its typed store
    const void* user; size_t bytes; int kind;
    bool staged; size_t off; void* dev;
  };
  template <class T> void add(T*& dev, const T* user, size_t count, int kind) {
    assert(n_ < MAX_ITEMS);
    items_[n_++] = Item{(void*)&dev, [](void* var, void* p) { *static_cast<T**>(var) = static_cast<T*>(p); }, user, count * sizeof(T), kind, false, 0, nullptr};
  }
  Backend be_;
  bool host_;
  Item items_[MAX_ITEMS];
  int n_ = 0;
};

}  // namespace myriad
