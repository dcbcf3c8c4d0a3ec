// One growing buffer carved into typed arrays: the placement arithmetic of every host-side workspace (ctx->rows, ctx->dnc,
// ctx->signguard, ...) and of the *_host entry points' staging area, written once.
//
//     Carve c;
//     c.take(&t.partials, chunks * n);      // nothing is bound yet
//     c.take(&t.keep, n);
//     BYZ_TRY(c.commit(ctx->dnc));          // ensure(total()), then every slot = base + its offset
//
// Every array starts on a kAlign = 16 byte boundary of the buffer, the first at its base: the base of a device buffer is at
// least 16-byte aligned (hipMalloc aligns to 256), so every array takes 16-byte vector loads and fp64 / int64 accesses whatever
// the length and element type of the arrays before it.  An array of no elements still gets an address of its own inside the
// buffer (one alignment unit).  Offsets are size_t formed from int64_t counts; a negative count, a byte size that overflows and
// a slot beyond kMaxSlots make commit() fail with BYZ_E_INVALID before it touches the buffer.  No heap allocation: the
// carvers run on every call of a hot loop.
// Plain C++17, no HIP: it also compiles with a host compiler (tests/carve_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/byzagg.h"

namespace byz {

void set_error(const char* fmt, ...);

class Carve {
  public:
    static constexpr int kMaxSlots = 32;
    static constexpr size_t kAlign = 16;
    static constexpr size_t kLimit = SIZE_MAX / 2;   // a layout ends below it: rounding a size up cannot wrap

    // *slot = the start of `count` elements of T once commit() has run
    template <typename T>
    void take(T** slot, int64_t count) {
        add(slot, [](void* s, char* p) { *static_cast<T**>(s) = reinterpret_cast<T*>(p); }, count, sizeof(T));
    }

    // Buf: byz::Buffer, or anything with `int ensure(size_t)` and `ptr`.  The only thing that touches the buffer.
    template <typename Buf>
    int commit(Buf& buf) {
        if (refused_ != nullptr) {
            set_error("workspace layout: %s (array %d)", refused_, n_slots_);
            return BYZ_E_INVALID;
        }
        const int rc = buf.ensure(total_);
        if (rc != BYZ_OK) return rc;
        char* base = static_cast<char*>(buf.ptr);
        for (int i = 0; i < n_slots_; ++i) slots_[i].bind(slots_[i].slot, base + slots_[i].offset);
        return BYZ_OK;
    }

    size_t total() const { return total_; }
    int slots() const { return n_slots_; }                            // arrays taken so far: the next take()'s index
    size_t offset(int index) const { return slots_[index].offset; }   // where array `index` starts in the buffer

  private:
    struct Slot {
        void* slot;
        void (*bind)(void* slot, char* address);
        size_t offset;
    };

    void add(void* slot, void (*bind)(void*, char*), int64_t count, size_t elem) {
        if (refused_ != nullptr) return;   // (n_slots_ stays at the first refused array)
        if (n_slots_ == kMaxSlots) refused_ = "more arrays than the table holds";
        else if (count < 0) refused_ = "negative element count";
        else if (total_ > kLimit || static_cast<uint64_t>(count) > (kLimit - total_) / elem) refused_ = "byte size overflows";
        if (refused_ != nullptr) return;
        const size_t bytes = static_cast<size_t>(count) * elem;
        slots_[n_slots_++] = {slot, bind, total_};
        total_ += (bytes == 0 ? kAlign : (bytes + kAlign - 1) / kAlign * kAlign);
    }

    Slot slots_[kMaxSlots];
    int n_slots_ = 0;
    size_t total_ = 0;
    const char* refused_ = nullptr;
};

}  // namespace byz
