// Stand-alone check of AlmLdsTable (csrc/launch.hpp), the bookkeeping behind alm_lds_limit: built by tests/test_launch_table.py with the host compiler
// and -fsanitize=address,undefined (no HIP: the header's HIP layer is compiled by hipcc only), run as a child process.  Exit code 0 = every check held.
#include <cstdio>
#include <thread>

#include "launch.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static int k0(int x) { return x; }           // four functions of ONE type (distinct bodies: never folded into one address)
static int k1(int x) { return x + 1; }
static int k2(int x) { return x + 2; }
static int k3(int x) { return x + 3; }

static const void* vp(int (*f)(int)) { return reinterpret_cast<const void*>(f); }

int main() {
    {   // (a) the attribute is per device: one pointer on device 0, then on device 1
        AlmLdsTable t;
        CHECK(t.needs_set(vp(k0), 0, 163840));
        t.record(vp(k0), 0, 163840);
        CHECK(t.needs_set(vp(k0), 1, 163840));
        t.record(vp(k0), 1, 163840);
        CHECK(!t.needs_set(vp(k0), 0, 163840));
        CHECK(!t.needs_set(vp(k0), 1, 163840));
        CHECK(t.size() == 2);
    }
    {   // (b) two pointers of one type are independent
        AlmLdsTable t;
        t.record(vp(k0), 0, 131072);
        CHECK(!t.needs_set(vp(k0), 0, 131072));
        CHECK(t.needs_set(vp(k1), 0, 131072));
        t.record(vp(k1), 0, 131072);
        CHECK(!t.needs_set(vp(k1), 0, 131072));
        CHECK(t.size() == 2);
    }
    {   // (c) more bytes for a seen pair: set again; fewer: not (and the grant does not shrink)
        AlmLdsTable t;
        t.record(vp(k0), 0, 65536);
        CHECK(t.needs_set(vp(k0), 0, 163840));
        t.record(vp(k0), 0, 163840);
        CHECK(!t.needs_set(vp(k0), 0, 65536));
        t.record(vp(k0), 0, 65536);
        CHECK(!t.needs_set(vp(k0), 0, 163840));
        CHECK(t.size() == 1);
    }
    {   // (d) a failed set is not recorded: asked for again
        AlmLdsTable t;
        CHECK(t.needs_set(vp(k0), 0, 163840));
        CHECK(t.needs_set(vp(k0), 0, 163840));
        CHECK(t.size() == 0);
    }
    {   // (e) 8 threads x 1000 calls over 4 pointers x 2 devices: exactly 8 entries, none needs a set afterwards
        AlmLdsTable t;
        const void* fns[4] = {vp(k0), vp(k1), vp(k2), vp(k3)};
        std::thread th[8];
        for (int i = 0; i < 8; ++i)
            th[i] = std::thread([&t, &fns, i] {
                for (int c = 0; c < 1000; ++c) {
                    const void* fn = fns[(c + i) & 3];
                    const int dev = ((c + i) >> 2) & 1;
                    if (t.needs_set(fn, dev, 163840)) t.record(fn, dev, 163840);
                }
            });
        for (std::thread& x : th) x.join();
        CHECK(t.size() == 8);
        for (int f = 0; f < 4; ++f)
            for (int dev = 0; dev < 2; ++dev) CHECK(!t.needs_set(fns[f], dev, 163840));
    }
    std::printf("ok\n");
    return 0;
}
