// orbx_lds_pollute.hpp - the test aid "lds_pollute" as a launcher sees it.  A launch* function takes an LdsPolluter by value as its last
// parameter and calls it in front of EVERY kernel it enqueues, the second and later ones included: LDS handed from one kernel of an entry to
// the next is exactly the accident the aid excludes.  The default one does nothing and a kernel file names no symbol of another (its host-compiled
// copies link alone), so a launcher knows no handle and, with the aid off, enqueues what it always did.  The host files make theirs from the handle (orbx_internal.hpp: ldsPolluter, polluteLds).
#pragma once
#include <hip/hip_runtime.h>

namespace orbx {
struct LdsPolluter {
    void (*launch)(hipStream_t, int, int, unsigned*) = nullptr;      // launchLdsPollute (k_gray.hip); null: the aid is off
    int numCUs = 0, byte = -1;
    unsigned* sink = nullptr;       // the handle's d_sink
    int* launches = nullptr;        // the handle's count of pollution launches (orbx_debug_lds_pollutions)
    void operator()(hipStream_t st) const {
        if (!launch || byte < 0) return;
        launch(st, numCUs, byte, sink);
        if (launches) ++*launches;
    }
};
}  // namespace orbx
