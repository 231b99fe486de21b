// Helper of make_depth_limit_golden.py (compiled by it with g++ into a temporary directory; not part of build()).
//
//   dl_real         the call sequence of torch.topk(largest=False) on the CPU (ATen/native/TopKImpl.h; the twin of
//                   oracle/vc2_oracle.cpp topk_smallest) with the REAL std::nth_element / std::sort / std::partial_sort,
//                   returning the whole permutation and the number of comparisons
//   dl_trace        an instrumented transcription of libstdc++'s __introselect / __introsort_loop / heap pieces that
//                   records whether and where the depth limits are met
//   dl_antiqs_*     the two adversaries (see the generator's docstring); their victim is the real std:: code
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <random>
#include <utility>
#include <vector>

namespace {

using elem_t = std::pair<float, int64_t>;
long g_ncmp = 0;
inline bool less_nan_last(const elem_t& x, const elem_t& y) {
  ++g_ncmp;
  return ((!std::isnan(x.first) && std::isnan(y.first)) || (x.first < y.first));
}

// ---------------------------------------------------------------- transcription (bits/stl_algo.h, bits/stl_heap.h)
struct Trace {
  int sel_hit = 0, sel_len = 0, sel_parts = 0, sel_pops = 0;       // __introselect: depth limit met, with which range; partitions made
  std::vector<int> seg_first, seg_last;              // __introsort_loop: every segment heap-sorted at depth 0
};
// (the comparator: torch's, or an adversary's; the hook: called when __introselect meets its depth limit)
bool (*g_cmp)(const elem_t&, const elem_t&) = nullptr;
void (*g_at_limit)() = nullptr;
inline bool cmp(const elem_t& x, const elem_t& y) { return g_cmp ? g_cmp(x, y) : less_nan_last(x, y); }
using It = elem_t*;
// 1: __adjust_heap takes the OTHER child when the two are equal -- a deliberately wrong heap step.  The generator asks which
// fixtures would notice (the answer changes) and prefers those: a fixture that no slip can change checks nothing.
int g_flip = 0;
inline bool lt(It a, It b) { return cmp(*a, *b); }

void t_push_heap(It first, long hole, long top, elem_t value) {
  long parent = (hole - 1) / 2;
  while (hole > top && cmp(first[parent], value)) {
    first[hole] = first[parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  first[hole] = value;
}
void t_adjust_heap(It first, long hole, long len, elem_t value) {
  const long top = hole;
  long child = hole;
  while (child < (len - 1) / 2) {
    child = 2 * (child + 1);
    if (g_flip ? !lt(first + (child - 1), first + child) : lt(first + child, first + (child - 1))) child--;
    first[hole] = first[child];
    hole = child;
  }
  if ((len & 1) == 0 && child == (len - 2) / 2) {
    child = 2 * (child + 1);
    first[hole] = first[child - 1];
    hole = child - 1;
  }
  t_push_heap(first, hole, top, value);
}
void t_make_heap(It first, It last) {
  if (last - first < 2) return;
  const long len = last - first;
  long parent = (len - 2) / 2;
  while (true) {
    elem_t value = first[parent];
    t_adjust_heap(first, parent, len, value);
    if (parent == 0) return;
    parent--;
  }
}
void t_pop_heap(It first, It last, It result) {
  elem_t value = *result;
  *result = *first;
  t_adjust_heap(first, 0, last - first, value);
}
long g_pops = 0;                                     // elements __heap_select took into the heap after __make_heap
void t_heap_select(It first, It middle, It last) {
  t_make_heap(first, middle);
  for (It i = middle; i < last; ++i)
    if (lt(i, first)) { ++g_pops; t_pop_heap(first, middle, i); }
}
void t_sort_heap(It first, It last) {
  while (last - first > 1) {
    --last;
    t_pop_heap(first, last, last);
  }
}
void t_move_median_to_first(It result, It a, It b, It c) {
  if (lt(a, b)) {
    if (lt(b, c)) std::iter_swap(result, b);
    else if (lt(a, c)) std::iter_swap(result, c);
    else std::iter_swap(result, a);
  } else if (lt(a, c)) std::iter_swap(result, a);
  else if (lt(b, c)) std::iter_swap(result, c);
  else std::iter_swap(result, b);
}
It t_unguarded_partition(It first, It last, It pivot) {
  while (true) {
    while (lt(first, pivot)) ++first;
    --last;
    while (lt(pivot, last)) --last;
    if (!(first < last)) return first;
    std::iter_swap(first, last);
    ++first;
  }
}
It t_partition_pivot(It first, It last) {
  It mid = first + (last - first) / 2;
  t_move_median_to_first(first, first + 1, mid, last - 1);
  return t_unguarded_partition(first + 1, last, first);
}
void t_unguarded_linear_insert(It last) {
  elem_t val = *last;
  It next = last;
  --next;
  while (cmp(val, *next)) {
    *last = *next;
    last = next;
    --next;
  }
  *last = val;
}
void t_insertion_sort(It first, It last) {
  if (first == last) return;
  for (It i = first + 1; i != last; ++i) {
    if (lt(i, first)) {
      elem_t val = *i;
      std::move_backward(first, i, i + 1);
      *first = val;
    } else
      t_unguarded_linear_insert(i);
  }
}
inline long lg(long n) { long r = 0; while (n > 1) { n >>= 1; ++r; } return r; }

void t_introselect(It first, It nth, It last, long depth, Trace& T) {
  while (last - first > 3) {
    if (depth == 0) {
      T.sel_hit = 1;
      T.sel_len = int(last - first);
      g_pops = 0;
      if (g_at_limit) g_at_limit();
      t_heap_select(first, nth + 1, last);
      T.sel_pops = int(g_pops);
      std::iter_swap(first, nth);
      return;
    }
    --depth;
    ++T.sel_parts;
    It cut = t_partition_pivot(first, last);
    if (cut <= nth) first = cut;
    else last = cut;
  }
  t_insertion_sort(first, last);
}
void t_introsort_loop(It base, It first, It last, long depth, Trace& T) {
  while (last - first > 16) {
    if (depth == 0) {
      T.seg_first.push_back(int(first - base));
      T.seg_last.push_back(int(last - base));
      t_heap_select(first, last, last);              // __partial_sort(first, last, last)
      t_sort_heap(first, last);
      return;
    }
    --depth;
    It cut = t_partition_pivot(first, last);
    t_introsort_loop(base, cut, last, depth, T);
    last = cut;
  }
}
void t_sort(It first, It last, Trace& T) {
  if (first == last) return;
  t_introsort_loop(first, first, last, lg(last - first) * 2, T);
  if (last - first > 16) {
    t_insertion_sort(first, first + 16);
    for (It i = first + 16; i != last; ++i) t_unguarded_linear_insert(i);
  } else
    t_insertion_sort(first, last);
}

// ---------------------------------------------------------------- the adversaries
// Elements are (0.f, id) pairs; the comparator answers from the adversary's state, keyed on the id.
struct Adv {
  std::vector<int64_t> major, minor;                 // value of id = (major, minor), compared lexicographically
  int64_t nfrozen = 0, candidate = -1;
  std::vector<std::vector<int32_t>> partners;        // phase 1 of the sort adversary: who met whom
  bool record = false;
  long ncmp = 0;
};
Adv* g_adv = nullptr;
constexpr int64_t kGas = INT64_MAX;

bool adv_less(const elem_t& ex, const elem_t& ey) {    // McIlroy's rule among the gas of one major
  Adv& A = *g_adv;
  ++A.ncmp;
  const int64_t x = ex.second, y = ey.second;
  if (x == y) return false;
  if (A.record) { A.partners[size_t(x)].push_back(int32_t(y)); A.partners[size_t(y)].push_back(int32_t(x)); }
  const bool gx = A.minor[size_t(x)] == kGas, gy = A.minor[size_t(y)] == kGas;
  if (gx && gy && A.major[size_t(x)] == A.major[size_t(y)]) {
    if (x == A.candidate) A.minor[size_t(x)] = A.nfrozen++;
    else A.minor[size_t(y)] = A.nfrozen++;
  }
  if (A.minor[size_t(x)] == kGas) A.candidate = x;
  else if (A.minor[size_t(y)] == kGas) A.candidate = y;
  if (A.major[size_t(x)] != A.major[size_t(y)]) return A.major[size_t(x)] < A.major[size_t(y)];
  return A.minor[size_t(x)] < A.minor[size_t(y)];
}
// distinct ranks 0 .. n-1 in the order of (major, minor, id); left-over gas counts as the largest of its major
void adv_ranks(const Adv& A, int n, int32_t* rank) {
  std::vector<int32_t> ids;
  ids.resize(size_t(n));
  for (int i = 0; i < n; ++i) ids[size_t(i)] = i;
  std::sort(ids.begin(), ids.end(), [&](int32_t a, int32_t b) {
    if (A.major[size_t(a)] != A.major[size_t(b)]) return A.major[size_t(a)] < A.major[size_t(b)];
    if (A.minor[size_t(a)] != A.minor[size_t(b)]) return A.minor[size_t(a)] < A.minor[size_t(b)];
    return a < b;
  });
  for (int r = 0; r < n; ++r) rank[ids[size_t(r)]] = r;
}

}  // namespace

extern "C" {

// perm[n]: the original index at every position after the calls; returns the number of comparisons
long dl_real(const float* v, int n, int k, int sorted, int64_t* perm) {
  std::vector<elem_t> q;
  q.resize(size_t(n));
  for (int j = 0; j < n; ++j) q[size_t(j)] = {v[j], j};
  g_ncmp = 0;
  if (int64_t(k) * 64 <= n) {
    std::partial_sort(q.begin(), q.begin() + k, q.end(), less_nan_last);
  } else {
    std::nth_element(q.begin(), q.begin() + (k - 1), q.end(), less_nan_last);
    if (sorted) std::sort(q.begin(), q.begin() + (k - 1), less_nan_last);
  }
  for (int j = 0; j < n; ++j) perm[j] = q[size_t(j)].second;
  return g_ncmp;
}

// the same through the transcription.  cert[0] = select depth limit met, cert[1] = its range length, cert[2] = partitions
// of the selection, cert[4] = elements its __heap_select took in after __make_heap, cert[3] = number of heap-sorted sort segments (the first `maxseg` of them in seg_first / seg_last)
long dl_trace(const float* v, int n, int k, int sorted, int64_t* perm, int32_t* cert, int32_t* seg_first, int32_t* seg_last,
              int maxseg, int flip) {
  g_flip = flip;
  std::vector<elem_t> q;
  q.resize(size_t(n));
  for (int j = 0; j < n; ++j) q[size_t(j)] = {v[j], j};
  Trace T;
  g_ncmp = 0;
  It b = q.data();
  if (int64_t(k) * 64 <= n) {
    t_heap_select(b, b + k, b + n);
    t_sort_heap(b, b + k);
  } else {
    if (n > 0 && k - 1 < n) t_introselect(b, b + (k - 1), b + n, lg(n) * 2, T);
    if (sorted) t_sort(b, b + (k - 1), T);
  }
  for (int j = 0; j < n; ++j) perm[j] = q[size_t(j)].second;
  g_flip = 0;
  cert[0] = T.sel_hit; cert[1] = T.sel_len; cert[2] = T.sel_parts; cert[3] = int(T.seg_first.size()); cert[4] = T.sel_pops;
  for (int s = 0; s < int(T.seg_first.size()) && s < maxseg; ++s) { seg_first[s] = T.seg_first[size_t(s)]; seg_last[s] = T.seg_last[size_t(s)]; }
  return g_ncmp;
}

// McIlroy's adversary against std::nth_element(q, q + k - 1, q + n) on the identity arrangement: rank[id], distinct
long dl_antiqs_select(int n, int k, int32_t* rank) {
  Adv A;
  A.major.assign(size_t(n), 0);
  A.minor.assign(size_t(n), kGas);
  g_adv = &A;
  std::vector<elem_t> q;
  q.resize(size_t(n));
  for (int j = 0; j < n; ++j) q[size_t(j)] = {0.f, j};
  std::nth_element(q.begin(), q.begin() + (k - 1), q.end(), adv_less);
  g_adv = nullptr;
  adv_ranks(A, n, rank);
  return A.ncmp;
}

// McIlroy's adversary up to the depth limit, then every value that is still gas gets its place in a seeded random order (gas
// has only ever been called larger than something solid: any values above the solid ones keep every answer given so far), so
// that the __heap_select of the fall-back has work to do.  The victim is the transcription: it knows where the limit is.
long dl_antiqs_select_busy(int n, int k, unsigned seed, int32_t* rank) {
  Adv A;
  A.major.assign(size_t(n), 0);
  A.minor.assign(size_t(n), kGas);
  g_adv = &A;
  static std::mt19937 rng;
  rng.seed(seed);
  g_cmp = adv_less;
  g_at_limit = [] {
    Adv& B = *g_adv;
    std::vector<int32_t> gas;
    for (size_t i = 0; i < B.minor.size(); ++i) if (B.minor[i] == kGas) gas.push_back(int32_t(i));
    for (size_t i = gas.size(); i > 1; --i) std::swap(gas[i - 1], gas[size_t(rng() % uint32_t(i))]);     // Fisher-Yates
    for (int32_t id : gas) B.minor[size_t(id)] = B.nfrozen++;
  };
  std::vector<elem_t> q;
  q.resize(size_t(n));
  for (int j = 0; j < n; ++j) q[size_t(j)] = {0.f, j};
  Trace T;
  t_introselect(q.data(), q.data() + (k - 1), q.data() + n, lg(n) * 2, T);
  g_cmp = nullptr;
  g_at_limit = nullptr;
  g_adv = nullptr;
  adv_ranks(A, n, rank);
  return A.ncmp;
}

// the two-phase adversary against nth_element + sort: sigma[id] is a permutation of 0 .. n-1
long dl_antiqs_sort(int n, int k, const int32_t* sigma, int hub_min, int32_t* rank, int32_t* nfree_out) {
  Adv A;
  A.major.assign(size_t(n), 0);
  A.minor.assign(size_t(n), 0);
  for (int i = 0; i < n; ++i) A.major[size_t(i)] = 2 * int64_t(sigma[i]);
  A.partners.assign(size_t(n), std::vector<int32_t>());
  A.record = true;
  g_adv = &A;
  std::vector<elem_t> q;
  q.resize(size_t(n));
  for (int j = 0; j < n; ++j) q[size_t(j)] = {0.f, j};
  std::nth_element(q.begin(), q.begin() + (k - 1), q.end(), adv_less);          // phase 1: answered from sigma
  A.record = false;
  std::vector<char> hub;
  hub.resize(size_t(n));
  for (int i = 0; i < n; ++i) {
    auto& p = A.partners[size_t(i)];
    std::sort(p.begin(), p.end());
    p.erase(std::unique(p.begin(), p.end()), p.end());
    hub[size_t(i)] = int(p.size()) >= hub_min;
  }
  std::vector<int64_t> hubs;                                                     // sigma of the hubs, ascending
  for (int i = 0; i < n; ++i) if (hub[size_t(i)]) hubs.push_back(sigma[i]);
  std::sort(hubs.begin(), hubs.end());
  int nfree = 0;
  for (int i = 0; i < n; ++i) {
    if (hub[size_t(i)]) continue;
    bool all_hubs = true;
    for (int32_t p : A.partners[size_t(i)]) all_hubs = all_hubs && hub[size_t(p)];
    if (!all_hubs) continue;
    // free again: gas above every solid of the sigma interval between the two hubs around it
    auto up = std::upper_bound(hubs.begin(), hubs.end(), int64_t(sigma[i]));
    const int64_t upper = up == hubs.end() ? int64_t(n) : *up;
    A.major[size_t(i)] = 2 * upper - 1;
    A.minor[size_t(i)] = kGas;
    ++nfree;
  }
  *nfree_out = nfree;
  A.candidate = -1;
  std::sort(q.begin(), q.begin() + (k - 1), adv_less);                           // phase 2: McIlroy's rule per interval
  g_adv = nullptr;
  adv_ranks(A, n, rank);
  return A.ncmp;
}

}  // extern "C"
