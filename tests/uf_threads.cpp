// The union-find of csrc/ef_unionfind.hpp on host threads: the text the device runs (k_comp_hook), with the compiler's __atomic builtins as
// its atomic operations.  Sixteen threads unite the edges of a chain (three row orders) and of a sheet, dealt round-robin, on one shared
// parent array; the labels must equal a sequential union-find's, every root must be its set's smallest row, and no loop may reach its cap.
// Built with -fsanitize=thread where the runtime is present (tests/test_components_host.py), the run also shows that no access to parent is
// a plain one.  Prints "ok <cases>" and returns 0, or says what differs and returns 1.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <thread>
#include <utility>
#include <vector>

#include "ef_unionfind.hpp"

namespace {

struct UfHost {
  static uint32_t load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
  static uint32_t cas(uint32_t* p, uint32_t expect, uint32_t want) {
    __atomic_compare_exchange_n(p, &expect, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expect;   // the value found, whether or not it matched
  }
  static void lower(uint32_t* p, uint32_t v) {
    uint32_t seen = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < seen && !__atomic_compare_exchange_n(p, &seen, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
  }
};

using Edge = std::pair<uint32_t, uint32_t>;

// rows along a line: row i stands at place[i]; an edge joins the rows of neighbouring places
std::vector<Edge> chain_edges(const std::vector<uint32_t>& place) {
  std::vector<uint32_t> row_at(place.size());
  for (uint32_t i = 0; i < place.size(); ++i) row_at[place[i]] = i;
  std::vector<Edge> e;
  for (uint32_t k = 0; k + 1 < place.size(); ++k) e.emplace_back(row_at[k], row_at[k + 1]);
  return e;
}
// an m x m grid with its eight-neighbourhood (spacing 0.7 r: the diagonal is within r), rows shuffled by perm
std::vector<Edge> sheet_edges(uint32_t m, const std::vector<uint32_t>& perm) {
  std::vector<Edge> e;
  for (uint32_t y = 0; y < m; ++y)
    for (uint32_t x = 0; x < m; ++x)
      for (int dy = 0; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if (dy == 0 && dx <= 0) continue;
          const int xx = (int)x + dx, yy = (int)y + dy;
          if (xx < 0 || xx >= (int)m || yy >= (int)m) continue;
          e.emplace_back(perm[y * m + x], perm[(uint32_t)yy * m + (uint32_t)xx]);
        }
  return e;
}
std::vector<uint32_t> shuffled(uint32_t n, uint32_t seed) {
  std::vector<uint32_t> p(n);
  std::iota(p.begin(), p.end(), 0u);
  uint64_t s = seed * 2654435761ull + 1;
  for (uint32_t i = n; i > 1; --i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    std::swap(p[i - 1], p[(uint32_t)((s >> 33) % i)]);
  }
  return p;
}

std::vector<uint32_t> sequential(uint32_t n, const std::vector<Edge>& edges) {
  std::vector<uint32_t> parent(n);
  std::iota(parent.begin(), parent.end(), 0u);
  auto find = [&](uint32_t x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  for (const Edge& e : edges) {
    const uint32_t a = find(e.first), b = find(e.second);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);
  }
  std::vector<uint32_t> label(n);
  for (uint32_t x = 0; x < n; ++x) label[x] = find(x);
  return label;
}

bool run(const char* name, uint32_t n, const std::vector<Edge>& edges, int threads, uint32_t extra_roots) {
  std::vector<uint32_t> parent(n);
  std::iota(parent.begin(), parent.end(), 0u);
  std::atomic<int> tripped{0};
  const uint32_t cap = n + 64u;
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t] {
      for (size_t k = (size_t)t; k < edges.size(); k += (size_t)threads) {
        uint32_t root;
        if (!efm::uf_union<UfHost>(parent.data(), edges[k].first, edges[k].second, cap, &root)) tripped.store(1);
      }
    });
  for (std::thread& th : pool) th.join();
  if (tripped.load()) { std::printf("%s: a loop reached its cap\n", name); return false; }
  const std::vector<uint32_t> want = sequential(n, edges);
  uint32_t roots = 0;
  for (uint32_t x = 0; x < n; ++x) {
    if (parent[x] > x) { std::printf("%s: parent[%u] = %u is above its row\n", name, x, parent[x]); return false; }
    uint32_t r;
    if (!efm::uf_find<UfHost>(parent.data(), x, cap, &r)) { std::printf("%s: find(%u) reached its cap\n", name, x); return false; }
    if (r != want[x]) { std::printf("%s: label[%u] = %u, the sequential union-find says %u\n", name, x, r, want[x]); return false; }
    roots += r == x;
  }
  if (roots != 1u + extra_roots) { std::printf("%s: %u components\n", name, roots); return false; }
  if (want[n - 1] != 0u && extra_roots == 0) { std::printf("%s: the label is not the smallest row\n", name); return false; }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const int threads = argc > 1 ? std::atoi(argv[1]) : 16;
  const uint32_t n = 3000, m = 96;
  int cases = 0;
  std::vector<uint32_t> asc(n), desc(n);
  std::iota(asc.begin(), asc.end(), 0u);
  for (uint32_t i = 0; i < n; ++i) desc[i] = n - 1 - i;
  for (int rep = 0; rep < 3; ++rep) {   // (another interleaving each time)
    if (!run("chain ascending", n, chain_edges(asc), threads, 0)) return 1;
    if (!run("chain descending", n, chain_edges(desc), threads, 0)) return 1;
    if (!run("chain shuffled", n, chain_edges(shuffled(n, 7 + rep)), threads, 0)) return 1;
    if (!run("sheet", m * m, sheet_edges(m, shuffled(m * m, 9 + rep)), threads, 0)) return 1;
    // two sheets that share no edge: two components, each labelled by its own smallest row
    std::vector<Edge> two = sheet_edges(m, shuffled(m * m, 11 + rep));
    for (const Edge& e : sheet_edges(m, shuffled(m * m, 12 + rep))) two.emplace_back(e.first + m * m, e.second + m * m);
    if (!run("two sheets", 2 * m * m, two, threads, 1)) return 1;
    cases += 5;
  }
  std::printf("ok %d\n", cases);
  return 0;
}
