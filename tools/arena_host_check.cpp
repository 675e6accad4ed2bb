// Host check of the FlashSR scratch arena (csrc/egr_arena.h) against a straightforward model.  The arena never dereferences what it
// hands out, so the slab source here deals in address ranges, not memory.  Meant to be built with a host compiler under the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/arena_host_check.cpp -o arena_host_check
// Seeded random get / put sequences, sizes from 0 and 1 byte over exact multiples of 256 to several slabs.  After every operation:
// the block is 256-aligned, lies inside one slab and overlaps no live block; get took the smallest free block that fits, over all
// slabs, and asked the source only when none did.  After every block is returned each slab holds one free block of its full size, and
// replaying the sequence asks the source for nothing (asserted for requests up to one slab; see run_seed).  A source that refuses the 2 GiB request but grants the exact one yields an
// exact-size slab; one that refuses both yields null with `total` unchanged.  Exit status 0 = all pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <vector>

#include "../comfyui-egregora-audio-super-resolution_amd/csrc/egr_arena.h"

static const size_t GiB = (size_t)1 << 30;

struct World {                                   // what the source has handed out, and how often it was asked
    std::map<char*, size_t> slabs;
    uintptr_t next = (uintptr_t)1 << 40;
    long long asked = 0;
    size_t refuse_from = SIZE_MAX;               // requests of at least this many bytes are refused
};

struct FakeSlabs {
    World* w = nullptr;
    void* get(size_t bytes) {
        ++w->asked;
        if (bytes >= w->refuse_from) return nullptr;
        char* p = (char*)w->next;
        w->next += ((bytes + 255) & ~(size_t)255) + (1 << 20);   // a gap, so that neighbouring slabs never look like one range
        w->slabs[p] = bytes;
        return p;
    }
    void put(void* base) { w->slabs.erase((char*)base); }
};
typedef egr::Arena<FakeSlabs> Arena;

static uint64_t g_state;
static uint64_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return g_state >> 17;
}

// oversize: 3 % of the requests are larger than a slab (up to 5 GiB) and get an exact-size slab of their own
static size_t random_size(bool oversize) {
    const unsigned k = (unsigned)(rnd() % 100);
    static const size_t edge[] = {0, 1, 255, 256, 257, 511, 512};
    if (k < 10) return edge[rnd() % 7];
    if (k < 45) return 1 + rnd() % (64 << 10);
    if (k < 75) return 1 + rnd() % (256 << 20);
    if (k < 90) return 256 * (1 + rnd() % (1 << 16));            // exact multiples of 256
    if (k < 97 || !oversize) return 1 + rnd() % (2 * GiB);       // up to a whole slab
    return 2 * GiB + 1 + rnd() % (3 * GiB);
}

struct Op { bool get; size_t bytes; size_t victim; };           // put: index into the list of live blocks
struct Block { char* p; size_t bytes; };

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return false; } while (0)

// the smallest free range >= need over all slabs, from the model alone (0: none); *starts collects where ranges of that size begin
static size_t model_best_fit(const World& w, const std::map<char*, size_t>& live, size_t need, std::vector<char*>* starts) {
    size_t best = 0;
    starts->clear();
    auto range = [&](char* a, char* b) {
        const size_t n = (size_t)(b - a);
        if (n < need || (best && n > best)) return;
        if (n != best) starts->clear();
        best = n;
        starts->push_back(a);
    };
    for (auto& s : w.slabs) {
        char* at = s.first;
        char* const end = s.first + s.second;
        for (auto it = live.lower_bound(s.first); it != live.end() && it->first < end; ++it) {
            range(at, it->first);
            at = it->first + it->second;
        }
        range(at, end);
    }
    return best;
}

static bool run_ops(Arena& arena, World& w, const std::vector<Op>& ops, bool may_ask, long long* n_ops) {
    std::map<char*, size_t> live;                // address -> rounded size
    std::vector<Block> blocks;
    std::vector<char*> starts;
    for (const Op& op : ops) {
        ++*n_ops;
        if (!op.get) {
            const Block b = blocks[op.victim % blocks.size()];
            blocks[op.victim % blocks.size()] = blocks.back();
            blocks.pop_back();
            arena.put(b.p, b.bytes);
            live.erase(b.p);
            continue;
        }
        const size_t need = Arena::round_up(op.bytes);
        const size_t best = model_best_fit(w, live, need, &starts);
        const long long asked0 = w.asked;
        const size_t total0 = arena.total;
        char* p = (char*)arena.get(op.bytes);
        if (!p) FAIL("get(%zu) returned null", op.bytes);
        if (((uintptr_t)p & 255) != 0) FAIL("get(%zu): %p is not 256-aligned", op.bytes, (void*)p);
        auto sl = w.slabs.upper_bound(p);
        if (sl == w.slabs.begin()) FAIL("get(%zu): %p lies in no slab", op.bytes, (void*)p);
        --sl;
        if (p + need > sl->first + sl->second) FAIL("get(%zu): %p + %zu leaves its slab", op.bytes, (void*)p, need);
        auto nx = live.lower_bound(p);
        if (nx != live.end() && nx->first < p + need) FAIL("get(%zu): overlaps the live block behind", op.bytes);
        if (nx != live.begin()) { auto pv = nx; --pv; if (pv->first + pv->second > p) FAIL("get(%zu): overlaps the live block in front", op.bytes); }
        if (best) {                              // a free block fits: the smallest one, and the source is left alone
            if (w.asked != asked0 || arena.total != total0) FAIL("get(%zu): asked the source although %zu free bytes fit", op.bytes, best);
            bool found = false;
            for (char* s : starts) found = found || s == p;
            if (!found) FAIL("get(%zu): not the smallest free block that fits (%zu bytes)", op.bytes, best);
        } else {
            if (!may_ask) FAIL("get(%zu): the replay asked the slab source", op.bytes);
            const size_t want = need > 2 * GiB ? need : 2 * GiB;
            if (w.asked != asked0 + 1 || p != sl->first || sl->second != want || arena.total != total0 + want)
                FAIL("get(%zu): expected one new slab of %zu bytes, handed out from its base", op.bytes, want);
        }
        live[p] = need;
        blocks.push_back(Block{p, op.bytes});
    }
    if (!blocks.empty()) FAIL("sequence left %zu blocks live", blocks.size());
    if (arena.slabs.size() != w.slabs.size()) FAIL("arena holds %zu slabs, the source gave %zu", arena.slabs.size(), w.slabs.size());
    for (auto& s : arena.slabs) {                // everything returned: one free block per slab, of its full size
        auto it = w.slabs.find(s.base);
        if (it == w.slabs.end() || it->second != s.size) FAIL("arena slab %p unknown to the source", (void*)s.base);
        if (s.by_addr.size() != 1 || s.by_size.size() != 1 || s.by_addr.begin()->first != s.base || s.by_addr.begin()->second != s.size ||
            s.by_size.begin()->first != s.size || s.by_size.begin()->second != s.base)
            FAIL("slab %p (%zu bytes) does not hold exactly one free block of its size after all returns", (void*)s.base, s.size);
    }
    return true;
}

// One sequence, run and replayed on the same arena.  Requests up to one slab: the replay must ask the source for nothing.  With
// oversize requests mixed in that is no property of a best-fit arena (a block that had an exact-size slab to itself the first time can
// find it partly taken by smaller blocks the second time); the replay then runs under every other check and its requests are counted.
static bool run_seed(uint64_t seed, int n_gets, bool oversize, long long* n_ops, size_t* n_slabs, long long* replay_asked) {
    g_state = seed;
    std::vector<Op> ops;
    size_t n_live = 0;
    for (int made = 0; made < n_gets || n_live > 0;) {
        const bool get = made < n_gets && (n_live == 0 || rnd() % 160 >= n_live);   // about 80 blocks live in the steady state
        if (get) { ops.push_back(Op{true, random_size(oversize), 0}); ++made; ++n_live; }
        else { ops.push_back(Op{false, 0, (size_t)rnd()}); --n_live; }
    }
    World w;
    {
        Arena arena;
        arena.src.w = &w;
        if (!run_ops(arena, w, ops, true, n_ops)) return false;
        const long long asked = w.asked;
        if (!run_ops(arena, w, ops, oversize, n_ops)) return false;
        *replay_asked += w.asked - asked;
        *n_slabs += w.slabs.size();
    }
    if (!w.slabs.empty()) FAIL("the arena's destructor left %zu slabs with the source", w.slabs.size());
    return true;
}

static bool run_refusals() {
    World w;
    Arena arena;
    arena.src.w = &w;
    w.refuse_from = 2 * GiB;                     // memory is tight: no 2 GiB slab, but the exact size
    char* p = (char*)arena.get(1000);
    if (!p || w.asked != 2 || arena.total != 1024 || arena.slabs.size() != 1 || arena.slabs[0].size != 1024 || arena.slabs[0].base != p)
        FAIL("refused 2 GiB, granted exact: expected one 1024-byte slab after two requests (asked %lld, total %zu)", w.asked, arena.total);
    if (arena.get(3 * GiB) || arena.total != 1024 || arena.slabs.size() != 1) FAIL("a 3 GiB request was not refused cleanly");
    w.refuse_from = 0;                           // both refused
    const long long asked = w.asked;
    if (arena.get(4096) || w.asked != asked + 2 || arena.total != 1024 || arena.slabs.size() != 1)
        FAIL("both refused: expected null after two requests with total unchanged (asked %lld, total %zu)", w.asked - asked, arena.total);
    char* q = (char*)arena.get(0);               // what is held still serves: 1024 bytes = 1000 rounded up, then nothing
    if (q) FAIL("a 256-byte block came out of a slab that is fully handed out");
    arena.put(p, 1000);
    q = (char*)arena.get(0);
    if (q != p || arena.get(768) != p + 256 || arena.get(1)) FAIL("the returned exact-size slab does not split into 256 + 768");
    return true;
}

int main() {
    const int seeds = 12, gets = 3000;
    long long n_ops = 0, replay_asked[2] = {0, 0};
    size_t n_slabs = 0;
    int bad = 0;
    for (int s = 0; s < 2 * seeds; ++s)          // every seed twice: requests up to one slab, then with oversize requests mixed in
        if (!run_seed(0x9E3779B97F4A7C15ull * (uint64_t)(s / 2 + 1), gets, s % 2 != 0, &n_ops, &n_slabs, &replay_asked[s % 2])) {
            printf("seed %d (%s) FAILED\n", s / 2, s % 2 ? "oversize" : "up to one slab");
            ++bad;
        }
    if (!run_refusals()) { printf("refusal cases FAILED\n"); ++bad; }
    printf("%d seeds x 2 sequences, %lld operations checked (each sequence run and replayed), %zu slabs; slab requests in the replays: %lld "
           "(up to one slab, must be 0), %lld (with oversize requests, counted only)\n", seeds, n_ops, n_slabs, replay_asked[0], replay_asked[1]);
    printf(bad ? "FAILED: %d\n" : "all sequences and refusal cases pass\n", bad);
    return bad ? 1 : 0;
}
