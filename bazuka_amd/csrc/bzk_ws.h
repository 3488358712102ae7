// One call's temporaries in the context's grow-only workspace slab.  Every buffer is declared once (take); commit reserves exactly what was
// declared and points the declared variables into the slab, checking each against the slab's size.  While a committed layout is in scope the slab
// must not move: a second commit (or ws_reserve) on the same context is refused.  take / bytes / bind are plain arithmetic - the CPU harness
// (tests/host/ws_check.cpp) runs them; only commit (ctx.hip) touches the context.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct bzk_ctx;

namespace bzk {

int32_t ws_reserve(bzk_ctx* ctx, size_t bytes, const char* who);  // ctx.hip: grows the slab to >= bytes for the call `who`; only WsLayout::commit calls it

struct WsLayout {
    static constexpr size_t ALIGN = 256, MAX_BUFS = 64;
    explicit WsLayout(const char* who) : who_(who) {}
    WsLayout(const WsLayout&) = delete;
    WsLayout& operator=(const WsLayout&) = delete;
    ~WsLayout() { if (live_) *live_ = nullptr; }
    // p will point at `count` elements, 256-byte aligned, once the layout is committed; until then (and when never taken) it is null
    template <class T>
    void take(T*& p, size_t count) {
        p = nullptr;
        add(&p, [](void* var, char* at) { *(T**)var = (T*)at; }, sizeof(T), count);
    }
    void add(void* var, void (*set)(void*, char*), size_t elem, size_t count) {
        const size_t off = (end_ + (ALIGN - 1)) & ~(ALIGN - 1);
        if (n_ == MAX_BUFS || off < end_ || (elem && count > (SIZE_MAX - off) / elem)) { bad_ = true; return; }
        buf_[n_++] = {var, set, off, elem * count};
        end_ = off + elem * count;
    }
    bool ok() const { return !bad_; }               // false: a size overflowed (or more than MAX_BUFS buffers)
    size_t bytes() const { return end_; }           // the last buffer's offset + its size
    size_t offset(size_t i) const { return buf_[i].off; }
    // points every declared variable into a slab of slab_bytes at base; false (nothing bound) when one would not fit
    bool bind(void* base, size_t slab_bytes) const {
        if (bad_) return false;
        for (size_t i = 0; i < n_; ++i)
            if (buf_[i].off > slab_bytes || buf_[i].bytes > slab_bytes - buf_[i].off) return false;
        for (size_t i = 0; i < n_; ++i) buf_[i].set(buf_[i].var, (char*)base + buf_[i].off);
        return true;
    }
    // instead of a slab: every declared variable gets alloc(its bytes), a block of its own (a CPU harness, whose sanitizer then sees each buffer's end)
    template <class A>
    void bind_each(A alloc) const {
        for (size_t i = 0; i < n_; ++i) buf_[i].set(buf_[i].var, (char*)alloc(buf_[i].bytes));
    }
    int32_t commit(bzk_ctx* ctx);  // ctx.hip: ws_reserve(bytes()), bind into ctx->ws; BZK_E_INTERNAL on a bad layout or inside another live one

private:
    struct Buf { void* var; void (*set)(void*, char*); size_t off, bytes; };
    const char* who_;
    const char** live_ = nullptr;  // &ctx->ws_live of the context this layout is committed on
    Buf buf_[MAX_BUFS];
    size_t n_ = 0, end_ = 0;
    bool bad_ = false;
};

}  // namespace bzk
