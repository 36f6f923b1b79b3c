// Workspace layouts of the image-side stages, host only.  A stage states its scratch planes once, in one layout function
// that walks a Carver over the caller's workspace: with a null base the same walk is the stage's *_workspace query.
#pragma once
#include "common.h"

namespace unetdc {

inline long align_up(long v, long a) { return (v + a - 1) / a * a; }

// Hands out typed planes from a base pointer (null: every plane is null); the running offset is the byte count.
class Carver {
 public:
  explicit Carver(void* base) : base_(static_cast<unsigned char*>(base)) {}
  // count elements of T at the running offset, which then moves on by their bytes rounded up to a multiple of `round`
  template <typename T> T* take(long count, long round = 1) {
    T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ += align_up(count * (long)sizeof(T), round);
    return p;
  }
  void align(long a) { off_ = align_up(off_, a); }
  void slack(long bytes) { off_ += bytes; }
  long bytes() const { return off_; }

 private:
  unsigned char* base_;
  long off_ = 0;
};

// What a layout function answers: whether the launcher accepts the geometry, the bytes the stage needs (0 when it does not)
// and the planes carved from the base it was given.
template <typename Planes> struct Layout {
  bool ok;
  long bytes;
  Planes planes;
};

// UNETDC_OK, or `code` with the message "<who>: workspace too small (<given> < <need> bytes)"
inline int require_workspace(const char* who, long given, long need, int code = UNETDC_EWORKSPACE) {
  if (given >= need) return UNETDC_OK;
  set_error("%s: workspace too small (%ld < %ld bytes)", who, given, need);
  return code;
}

}  // namespace unetdc
