// grammar.h -- grammar-constrained sampling on the host: a GBNF reader, an incremental matcher
// over Unicode code points and the allowed-token bit mask of a request's state.  No HIP: this compiles and runs
// without a GPU (tools/grammar_selfcheck.cpp builds it alone).
#pragma once
#include <atomic>
#include <cstdint>
#include <list>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

namespace mx {
namespace gram {

// a state may hold at most this many grammar positions (stacks) at once; past it the request ends with an error
constexpr size_t MAX_POSITIONS = 4096;
// the work one mask (or one accepted token) may take, in stack elements touched: past it the request ends with the
// same error.  It bounds the time a request can hold the scheduler thread whatever its grammar is
constexpr uint64_t WORK_BUDGET = 1u << 20;
// helper rules a repetition may be rewritten into, in elements over the whole grammar
constexpr size_t MAX_ELEMENTS = 1u << 16;

// The vocabulary a grammar is matched against: the piece bytes of every token and the end-of-generation ids.
// `order` lists the tokens with a non-empty piece that are not end-of-generation ids, sorted by piece bytes, so
// a range of it with a common prefix is a subtree of the vocabulary's byte trie.
struct Vocab {
  int n_vocab = 0;
  std::vector<uint8_t> blob;
  std::vector<uint64_t> off;  // [n_vocab + 1]
  std::vector<int32_t> eog;
  std::vector<uint8_t> is_eog;  // [n_vocab]
  std::vector<int32_t> order;
  const uint8_t* piece(int t) const { return blob.data() + off[t]; }
  size_t len(int t) const { return (size_t)(off[t + 1] - off[t]); }
  // empty string on success, else what is wrong
  static std::string create(int n_vocab, const uint8_t* blob, const uint64_t* offsets, const int32_t* eog, int n_eog,
                            std::shared_ptr<const Vocab>* out);
};

// a set of code points: sorted, merged inclusive ranges, possibly negated
struct CharClass {
  bool negated = false;
  std::vector<std::pair<uint32_t, uint32_t>> ranges;
  bool has(uint32_t c) const;
  bool hits(uint32_t lo, uint32_t hi) const;  // some code point of [lo, hi] is in the set
};

struct Elem {
  int32_t ref = -1;  // >= 0: a rule
  int32_t cls = -1;  // >= 0: a class of Grammar::classes
};

// a position: alternative `alt` of Grammar::alts, element `idx` of it
struct Pos {
  int32_t alt, idx;
  bool operator==(const Pos& o) const { return alt == o.alt && idx == o.idx; }
  bool operator<(const Pos& o) const { return alt != o.alt ? alt < o.alt : idx < o.idx; }
};
// what is still to be matched, innermost last; its last position is always a class element.  Empty: the grammar
// may end here.
typedef std::vector<Pos> Stack;

class Grammar {
 public:
  // parses and checks `text` (syntax, undefined rules, root, {m,n}, left recursion); empty string on success.
  // cache_entries: masks kept per grammar (0: no cache)
  static std::string create(std::shared_ptr<const Vocab> vocab, const char* text, int cache_entries,
                            std::shared_ptr<Grammar>* out);
  std::shared_ptr<const Vocab> vocab;
  std::vector<std::string> rule_names;
  std::vector<std::vector<int32_t>> rules;  // rule -> its alternatives (indices into alts)
  std::vector<std::vector<Elem>> alts;
  std::vector<CharClass> classes;
  int root = -1;

  // `st` with its innermost reference expanded until every stack ends in a class element, added to `out`
  // (sorted, unique).  false: more than MAX_POSITIONS stacks, or *work past WORK_BUDGET
  bool expand(const Stack& st, std::set<Stack>& seen, std::vector<Stack>& out, uint64_t* work) const;
  bool initial(std::vector<Stack>& out, uint64_t* work) const;
  // the stacks after code point c; false on overflow
  bool advance(const std::vector<Stack>& in, uint32_t c, std::vector<Stack>& out, uint64_t* work) const;
  // stack elements the last computed mask of this grammar touched (what WORK_BUDGET bounds)
  mutable std::atomic<uint64_t> last_work{0};
  bool hits(const std::vector<Stack>& in, uint32_t lo, uint32_t hi) const;

  // the mask of (stacks, pending bytes): from the cache, or computed by one walk of the vocabulary
  std::shared_ptr<const std::vector<uint32_t>> mask(const std::vector<Stack>& stacks, const std::string& pending);
  void stats(uint64_t* hits, uint64_t* misses, uint64_t* entries);

 private:
  void compute_mask(const std::vector<Stack>& stacks, const std::string& pending, std::vector<uint32_t>& words) const;
  struct Entry {
    std::string key;
    std::shared_ptr<const std::vector<uint32_t>> mask;
  };
  std::mutex mu;
  size_t cache_cap = 0;
  std::list<Entry> lru;  // most recently used first
  std::unordered_map<std::string, std::list<Entry>::iterator> index;
  uint64_t n_hits = 0, n_misses = 0;
};

// UTF-8 as the matcher reads it: strict (no overlong forms, no surrogates, nothing above U+10FFFF)
struct Utf8 {
  // the valid second-byte range after lead byte b0 and the sequence length; false: b0 cannot start a sequence
  static bool lead(uint8_t b0, int* len, uint8_t* lo2, uint8_t* hi2);
  // the code points whose encoding starts with the valid incomplete prefix p[0..n)
  static void range(const uint8_t* p, int n, uint32_t* lo, uint32_t* hi);
};

enum { STATE_OK = 0, STATE_DEAD_END = 1, STATE_CAP = 2 };

// One request's place in a grammar.  Holds the grammar alive.
class State {
 public:
  explicit State(std::shared_ptr<Grammar> g);
  // the allowed-token mask of the current state, ceil(V / 32) words.  STATE_OK, STATE_DEAD_END (no token allowed;
  // the words are all zero) or STATE_CAP (position cap exceeded; all zero)
  int mask(std::shared_ptr<const std::vector<uint32_t>>* out);
  // false: the token is not allowed here (the state is unchanged)
  bool accept(int32_t token);
  bool may_end() const;
  bool ended() const { return done; }
  const std::shared_ptr<Grammar>& grammar() const { return g; }

 private:
  std::shared_ptr<Grammar> g;
  std::vector<Stack> stacks;
  std::string pending;  // bytes of an unfinished UTF-8 sequence
  bool overflow = false, done = false;
};

}  // namespace gram
}  // namespace mx
