// TEST HARNESS (not product): the layout arithmetic of a call's workspace (bazuka_amd/csrc/bzk_ws.h) on the CPU.  Plain C++: the header's
// take / bytes / bind do not touch the HIP runtime.
#include "../../bazuka_amd/csrc/bzk_ws.h"

#include <vector>

extern "C" {
// n buffers of count[i] elements of elem[i] bytes are declared, off_out[i] receives their offsets and *bytes_out the size to reserve; then they
// are bound into a slab of slab_bytes (an address range only: nothing is dereferenced) and bound_out[i] receives each bound pointer's distance
// from the slab's base.  0: bound; 1: the slab is too short, nothing bound; 2: the layout itself was refused (a size overflows, more than
// WsLayout::MAX_BUFS buffers)
int ws_check_layout(const uint64_t* elem, const uint64_t* count, int n, uint64_t slab_bytes, uint64_t* off_out, uint64_t* bytes_out, uint64_t* bound_out) {
    bzk::WsLayout ws("ws_check_layout");
    std::vector<char*> var((size_t)n, nullptr);
    for (int i = 0; i < n; ++i) ws.add(&var[i], [](void* v, char* at) { *(char**)v = at; }, (size_t)elem[i], (size_t)count[i]);
    if (!ws.ok()) return 2;
    for (int i = 0; i < n; ++i) off_out[i] = ws.offset(i);
    *bytes_out = ws.bytes();
    char* const base = (char*)(uintptr_t)0x10000;
    if (!ws.bind(base, (size_t)slab_bytes)) {
        for (int i = 0; i < n; ++i)
            if (var[i]) return -1;  // a refused binding must leave every variable untouched
        return 1;
    }
    for (int i = 0; i < n; ++i) bound_out[i] = (uint64_t)(var[i] - base);
    return 0;
}
}
