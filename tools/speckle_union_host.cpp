// The union-find of csrc/speckle_union.h on the CPU, where a sanitizer can watch it: the same find / unite text the kernels of
// csrc/disparity_speckle.hip run, over a host array of std::atomic<int>, driven by several threads that take the links of a map in
// an interleaved order -- first inside tiles, then across them, as the launches do -- and compared with a sequential flood fill.
// Maps: the serpentine and the U across tiles of tests/speckle_cases.py, a constant map and a random one.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread tools/speckle_union_host.cpp -o /tmp/speckle_union_host && /tmp/speckle_union_host
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../semstereo_amd/csrc/speckle_union.h"

namespace {

constexpr int TH = 32, TW = 64, THREADS = 4;

struct HostParents {
    std::atomic<int>* p;
    int load(int i) const { return p[i].load(std::memory_order_relaxed); }
    int fetch_min(int i, int v) const {
        int old = p[i].load(std::memory_order_relaxed);
        while (old > v && !p[i].compare_exchange_weak(old, v, std::memory_order_relaxed)) {
        }
        return old;
    }
};

struct Link {
    int a, b;
};

// valid[p] != 0: a pixel; two valid 4-neighbours link if their levels are equal
int check(const char* what, int H, int W, const std::vector<int>& level) {
    const int n = H * W;
    std::vector<Link> inside, across;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int p = y * W + x;
            if (level[p] < 0) continue;
            if (x + 1 < W && level[p + 1] == level[p]) ((x + 1) % TW ? inside : across).push_back({p, p + 1});
            if (y + 1 < H && level[p + W] == level[p]) ((y + 1) % TH ? inside : across).push_back({p, p + W});
        }
    std::vector<std::atomic<int>> parent(n);
    for (int p = 0; p < n; ++p) parent[p].store(p);
    const HostParents m{parent.data()};
    for (const std::vector<Link>* links : {&inside, &across}) {
        std::vector<std::thread> pool;
        for (int t = 0; t < THREADS; ++t)
            pool.emplace_back([&, t] {
                for (size_t i = t; i < links->size(); i += THREADS) ss::speckle::unite(m, (*links)[i].a, (*links)[i].b);
            });
        for (auto& th : pool) th.join();
    }
    // the flood fill: the first pixel of a component in raster order is its smallest index
    std::vector<int> want(n, -1), stack;
    for (int first = 0; first < n; ++first) {
        if (level[first] < 0 || want[first] >= 0) continue;
        want[first] = first;
        stack.assign(1, first);
        while (!stack.empty()) {
            const int p = stack.back(), y = p / W, x = p % W;
            stack.pop_back();
            const int q[4] = {x + 1 < W ? p + 1 : -1, x > 0 ? p - 1 : -1, y + 1 < H ? p + W : -1, y > 0 ? p - W : -1};
            for (int k = 0; k < 4; ++k)
                if (q[k] >= 0 && want[q[k]] < 0 && level[q[k]] == level[p]) want[q[k]] = first, stack.push_back(q[k]);
        }
    }
    int bad = 0;
    for (int p = 0; p < n; ++p)
        if (level[p] >= 0 && ss::speckle::find(m, p) != want[p]) ++bad;
    std::printf("%-12s %4d x %-4d links %6zu + %-5zu %s\n", what, H, W, inside.size(), across.size(), bad ? "WRONG" : "ok");
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    {
        const int H = 2 * TH + 1, W = 2 * TW + 1;
        std::vector<int> v(H * W, -1);
        for (int y = 0; y < H; y += 2)
            for (int x = 0; x < W; ++x) v[y * W + x] = 1;
        for (int y = 1; y < H; y += 2) v[y * W + (y % 4 == 1 ? W - 1 : 0)] = 1;
        bad += check("serpentine", H, W, v);
    }
    {
        const int H = 2 * TH, W = TW;
        std::vector<int> v(H * W, -1);
        for (int y = 2; y < TH; ++y) v[y * W + 3] = v[y * W + 10] = 2;
        for (int x = 3; x <= 10; ++x) v[TH * W + x] = 2;
        bad += check("u", H, W, v);
    }
    {
        const int H = 4 * TH, W = 4 * TW;
        bad += check("constant", H, W, std::vector<int>(H * W, 0));
    }
    {
        const int H = 3 * TH + 5, W = 3 * TW + 7;
        std::vector<int> v(H * W);
        unsigned s = 12345u;
        for (int& x : v) s = s * 1664525u + 1013904223u, x = (int)(s >> 30) - 1;       // -1 (a hole), 0, 1, 2
        bad += check("random", H, W, v);
    }
    return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
