// Ownership of DevBuf and PinBuf (camkifu_amd/csrc/ck_buf.h) under ASan / UBSan, with leak detection: the header alone,
// over counting versions of its four allocator functions (malloc / free), no GPU runtime anywhere.  Checks that growing
// frees once and allocates once, that a request that fits does nothing, that a move leaves exactly one owner, that a
// vector of model-like structs survives its reallocations, that assigning an empty struct frees everything, and that at
// exit every allocation has been freed exactly once.  tools/sanitize/run.sh builds and runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <set>
#include <utility>
#include <vector>
#include "../../camkifu_amd/csrc/ck_buf.h"

static long g_dev_allocs, g_dev_frees, g_pin_allocs, g_pin_frees;
static unsigned g_last_flags;
static std::set<void*> g_live;                 // a second free of one block, or a free of a stranger, is caught here too

static int counted_alloc(void** p, size_t bytes, long* count)
{
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return 2;
    memset(*p, 0xA5, bytes);
    g_live.insert(*p);
    ++*count;
    return 0;
}
static int counted_free(void* p, long* count)
{
    if (!g_live.erase(p)) { printf("free of a block that is not live\n"); _exit(1); }
    free(p);
    ++*count;
    return 0;
}
int ck_dev_alloc(void** p, size_t bytes) { return counted_alloc(p, bytes, &g_dev_allocs); }
int ck_dev_free(void* p) { return counted_free(p, &g_dev_frees); }
int ck_pin_alloc(void** p, size_t bytes, unsigned flags) { g_last_flags = flags; return counted_alloc(p, bytes, &g_pin_allocs); }
int ck_pin_free(void* p) { return counted_free(p, &g_pin_frees); }

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); _exit(1); } \
    } while (0)

// the shape of Mog2State: four device buffers, one pinned, a flag
struct Model {
    DevBuf weight, variance, mean, nmodes;
    PinBuf rates;
    bool alive = false;
};

static void fill(Model& m, size_t bytes)
{
    CHECK(m.weight.reserve(bytes, bytes + 8) == 0 && m.variance.reserve(bytes, bytes + 8) == 0);
    CHECK(m.mean.reserve(3 * bytes, 3 * bytes) == 0 && m.nmodes.reserve(bytes / 4 + 1, bytes) == 0);
    CHECK(m.rates.reserve(64, 4096) == 0);
    m.alive = true;
}

template <class B>
static void grow_and_move(long& allocs, long& frees)
{
    const long a0 = allocs, f0 = frees;
    {
        B b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.reserve(100, 100 + 100 / 8 + 256) == 0);
        CHECK(b.p && b.cap == 368 && allocs == a0 + 1 && frees == f0);
        void* first = b.p;
        CHECK(b.reserve(368, 9999) == 0 && b.reserve(0, 1) == 0 && b.reserve(1, 1) == 0);     // within capacity: nothing
        CHECK(b.p == first && b.cap == 368 && allocs == a0 + 1 && frees == f0);
        CHECK(b.reserve(369, 1000) == 0);                                                       // past it: one free, one allocation
        CHECK(b.cap == 1000 && allocs == a0 + 2 && frees == f0 + 1);
        memset(b.p, 1, b.cap);
        B c(std::move(b));                                                                      // move construction
        CHECK(b.p == nullptr && b.cap == 0 && c.cap == 1000 && allocs == a0 + 2 && frees == f0 + 1);
        B d;
        CHECK(d.reserve(10, 10) == 0 && allocs == a0 + 3);
        void* held = c.p;
        d = std::move(c);                                                                       // move assignment: d's own block goes
        CHECK(c.p == nullptr && c.cap == 0 && d.p == held && d.cap == 1000 && frees == f0 + 2);
        B& self = d;
        d = std::move(self);                                                                    // onto itself: nothing
        CHECK(d.p == held && d.cap == 1000 && frees == f0 + 2);
        CHECK(b.release() == 0 && frees == f0 + 2);                                             // an empty buffer frees nothing
        CHECK(b.reserve(5, 5) == 0 && allocs == a0 + 4);                                        // and is usable again
    }
    CHECK(allocs == a0 + 4 && frees == f0 + 4);
}

int main()
{
    grow_and_move<DevBuf>(g_dev_allocs, g_dev_frees);
    grow_and_move<PinBuf>(g_pin_allocs, g_pin_frees);
    {
        PinBuf mapped(CK_PIN_MAPPED);
        CHECK(mapped.reserve(64, 64) == 0 && g_last_flags == CK_PIN_MAPPED);
        PinBuf moved(std::move(mapped));
        CHECK(moved.flags == CK_PIN_MAPPED && moved.cap == 64 && mapped.p == nullptr);
        PinBuf plain;
        CHECK(plain.reserve(8, 8) == 0 && g_last_flags == CK_PIN_DEFAULT);
    }
    CHECK(g_live.empty());

    // a vector of models through 100 reallocations: every element moves, nothing is freed, nothing is lost
    {
        const long a0 = g_dev_allocs, f0 = g_dev_frees, pa0 = g_pin_allocs, pf0 = g_pin_frees;
        std::vector<Model> models;
        std::vector<void*> weight_of;
        for (int i = 0; i < 100; i++) {
            models.shrink_to_fit();                          // capacity == size: the next emplace_back reallocates
            CHECK(models.capacity() == models.size());
            models.emplace_back();
            fill(models.back(), 40 + (size_t)i);
            weight_of.push_back(models.back().weight.p);
        }
        CHECK(g_dev_allocs == a0 + 400 && g_dev_frees == f0 && g_pin_allocs == pa0 + 100 && g_pin_frees == pf0);
        for (int i = 0; i < 100; i++) {
            const Model& m = models[(size_t)i];
            CHECK(m.alive && m.weight.p == weight_of[(size_t)i] && m.weight.cap == 48 + (size_t)i && m.rates.cap == 4096);
            CHECK(((unsigned char*)m.mean.p)[3 * (40 + i) - 1] == 0xA5);
        }
        // assigning an empty struct frees everything that one held, and only that
        models[7] = Model();
        CHECK(!models[7].alive && !models[7].weight.p && !models[7].variance.p && !models[7].mean.p && !models[7].nmodes.p && !models[7].rates.p);
        CHECK(g_dev_frees == f0 + 4 && g_pin_frees == pf0 + 1 && g_live.size() == 99 * 5);
        fill(models[7], 1000);                               // the slot is reusable
        CHECK(g_dev_allocs == a0 + 404 && g_pin_allocs == pa0 + 101);
        models.erase(models.begin() + 20, models.begin() + 60);      // move assignment down the vector
        CHECK(models.size() == 60 && models[20].weight.p == weight_of[60] && g_live.size() == 60 * 5);
    }
    CHECK(g_live.empty());
    CHECK(g_dev_allocs == g_dev_frees && g_pin_allocs == g_pin_frees);
    printf("ok: %ld device and %ld pinned allocations, all freed once\n", g_dev_allocs, g_pin_allocs);
    return 0;
}
