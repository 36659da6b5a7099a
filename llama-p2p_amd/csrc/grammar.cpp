// grammar.cpp -- GBNF reader, incremental matcher and allowed-token masks.  Host only.
//
// A grammar is a list of rules, each a list of alternatives, each a list of elements: a class of code points or
// a reference to a rule.  Literals are one single-point class per code point; groups and repetitions are
// rewritten into helper rules (right-recursive, so they are never left-recursive themselves).  A request's state
// is a set of stacks of positions still to be matched (innermost last), every stack ending in a class element;
// a code point advances the stacks whose class holds it and expands the references that come next.  The mask of
// a state walks the vocabulary sorted by piece bytes as a byte trie, carrying the stack set and the UTF-8
// decoder along every path and cutting a subtree as soon as no stack is left.
#include "grammar.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <set>
#include <unordered_map>

namespace mx {
namespace gram {

// ---------------------------------------------------------------- UTF-8

bool Utf8::lead(uint8_t b0, int* len, uint8_t* lo2, uint8_t* hi2) {
  *lo2 = 0x80, *hi2 = 0xBF;
  if (b0 < 0x80) return *len = 1, true;
  if (b0 >= 0xC2 && b0 <= 0xDF) return *len = 2, true;
  if (b0 >= 0xE0 && b0 <= 0xEF) {
    if (b0 == 0xE0) *lo2 = 0xA0;  // no overlong forms
    if (b0 == 0xED) *hi2 = 0x9F;  // no surrogates
    return *len = 3, true;
  }
  if (b0 >= 0xF0 && b0 <= 0xF4) {
    if (b0 == 0xF0) *lo2 = 0x90;
    if (b0 == 0xF4) *hi2 = 0x8F;  // nothing above U+10FFFF
    return *len = 4, true;
  }
  return false;
}

static uint32_t decode(const uint8_t* p, int n) {
  if (n == 1) return p[0];
  if (n == 2) return (uint32_t)(p[0] & 0x1F) << 6 | (p[1] & 0x3F);
  if (n == 3) return (uint32_t)(p[0] & 0x0F) << 12 | (uint32_t)(p[1] & 0x3F) << 6 | (p[2] & 0x3F);
  return (uint32_t)(p[0] & 0x07) << 18 | (uint32_t)(p[1] & 0x3F) << 12 | (uint32_t)(p[2] & 0x3F) << 6 | (p[3] & 0x3F);
}

void Utf8::range(const uint8_t* p, int n, uint32_t* lo, uint32_t* hi) {
  int len;
  uint8_t lo2, hi2, a[4], b[4];
  lead(p[0], &len, &lo2, &hi2);
  for (int i = 0; i < len; i++) {
    a[i] = i < n ? p[i] : i == 1 ? lo2 : 0x80;
    b[i] = i < n ? p[i] : i == 1 ? hi2 : 0xBF;
  }
  *lo = decode(a, len), *hi = decode(b, len);
}

// the decoder of a byte stream: 0..3 bytes of an unfinished sequence
struct Dec {
  uint8_t buf[4] = {0, 0, 0, 0};
  int n = 0, need = 0;
  uint8_t lo2 = 0x80, hi2 = 0xBF;
  // feeds one byte: -1 invalid, 0 inside a sequence, 1 a code point is complete (*cp)
  int feed(uint8_t b, uint32_t* cp) {
    if (n == 0) {
      if (!Utf8::lead(b, &need, &lo2, &hi2)) return -1;
      buf[0] = b, n = 1;
    } else {
      const uint8_t lo = n == 1 ? lo2 : 0x80, hi = n == 1 ? hi2 : 0xBF;
      if (b < lo || b > hi) return -1;
      buf[n++] = b;
    }
    if (n < need) return 0;
    *cp = decode(buf, need);
    n = 0;
    return 1;
  }
};

// ---------------------------------------------------------------- vocabulary

std::string Vocab::create(int n_vocab, const uint8_t* blob, const uint64_t* offsets, const int32_t* eog, int n_eog,
                          std::shared_ptr<const Vocab>* out) {
  if (n_vocab < 1 || !offsets || n_eog < 0 || (n_eog && !eog)) return "vocabulary: n_vocab >= 1, offsets and ids";
  if (offsets[0] != 0) return "vocabulary: offsets start at 0";
  for (int t = 0; t < n_vocab; t++) {
    if (offsets[t + 1] < offsets[t]) return "vocabulary: offsets decrease at token " + std::to_string(t);
    if (offsets[t + 1] - offsets[t] > 4096) return "vocabulary: the piece of token " + std::to_string(t) + " is longer than 4096 bytes";
  }
  if (offsets[n_vocab] && !blob) return "vocabulary: null piece bytes";
  auto v = std::make_shared<Vocab>();
  v->n_vocab = n_vocab;
  v->blob.assign(blob, blob + offsets[n_vocab]);
  v->off.assign(offsets, offsets + n_vocab + 1);
  v->is_eog.assign(n_vocab, 0);
  for (int i = 0; i < n_eog; i++) {
    if (eog[i] < 0 || eog[i] >= n_vocab) return "vocabulary: end-of-generation id out of range";
    if (!v->is_eog[eog[i]]) v->eog.push_back(eog[i]);
    v->is_eog[eog[i]] = 1;
  }
  for (int t = 0; t < n_vocab; t++)
    if (v->len(t) && !v->is_eog[t]) v->order.push_back(t);
  const Vocab* p = v.get();
  std::sort(v->order.begin(), v->order.end(), [p](int32_t a, int32_t b) {
    const size_t la = p->len(a), lb = p->len(b);
    const int c = memcmp(p->piece(a), p->piece(b), std::min(la, lb));
    if (c) return c < 0;
    return la != lb ? la < lb : a < b;
  });
  *out = v;
  return "";
}

// ---------------------------------------------------------------- classes

bool CharClass::has(uint32_t c) const {
  bool in = false;
  for (const auto& r : ranges)
    if (c >= r.first && c <= r.second) {
      in = true;
      break;
    }
  return in != negated;
}

bool CharClass::hits(uint32_t lo, uint32_t hi) const {
  uint64_t covered = 0;  // the ranges are merged, so they do not overlap
  for (const auto& r : ranges) {
    const uint32_t a = std::max(lo, r.first), b = std::min(hi, r.second);
    if (a <= b) covered += (uint64_t)b - a + 1;
  }
  return negated ? covered < (uint64_t)hi - lo + 1 : covered > 0;
}

static void normalize(CharClass& c) {
  std::sort(c.ranges.begin(), c.ranges.end());
  std::vector<std::pair<uint32_t, uint32_t>> m;
  for (const auto& r : c.ranges) {
    if (!m.empty() && (uint64_t)r.first <= (uint64_t)m.back().second + 1) m.back().second = std::max(m.back().second, r.second);
    else m.push_back(r);
  }
  c.ranges.swap(m);
}

// ---------------------------------------------------------------- GBNF reader

namespace {
struct ParseError {
  std::string msg;
};

struct Parser {
  Grammar& g;
  const char* src;
  const char* p;
  std::map<std::string, int> ids;
  std::vector<char> defined;
  std::vector<std::string> first_ref;  // the rule that first referred to each rule
  size_t n_elems = 0;
  int n_helpers = 0;

  Parser(Grammar& g_, const char* s) : g(g_), src(s), p(s) {}

  [[noreturn]] void die(const std::string& what, const std::string& rule = "") const {
    int line = 1, col = 1;
    for (const char* q = src; q < p; q++) {
      if (*q == '\n') line++, col = 1;
      else col++;
    }
    throw ParseError{"grammar: " + what + (rule.empty() ? "" : " in rule '" + rule + "'") + " at line " +
                     std::to_string(line) + ", column " + std::to_string(col)};
  }
  static bool word(char c) {
    return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '-' || c == '_';
  }
  void space(bool newline_ok) {
    for (;;) {
      if (*p == ' ' || *p == '\t' || (newline_ok && (*p == '\r' || *p == '\n'))) p++;
      else if (*p == '#') {
        while (*p && *p != '\r' && *p != '\n') p++;
      } else return;
    }
  }
  int rule_id(const std::string& name) {
    auto it = ids.find(name);
    if (it != ids.end()) return it->second;
    const int id = (int)g.rules.size();
    ids[name] = id;
    g.rule_names.push_back(name);
    g.rules.emplace_back();
    defined.push_back(0);
    first_ref.emplace_back();
    return id;
  }
  int helper(const std::string& parent) {
    const int id = rule_id(parent + "#" + std::to_string(++n_helpers));  // '#' is in no written name
    defined[id] = 1;
    return id;
  }
  void add_alt(int rule, std::vector<Elem> a) {
    n_elems += a.size() + 1;
    if (n_elems > MAX_ELEMENTS) die("the grammar is too large (repetition counts)", g.rule_names[rule]);
    g.rules[rule].push_back((int32_t)g.alts.size());
    g.alts.push_back(std::move(a));
  }
  std::string name() {
    const char* b = p;
    while (word(*p)) p++;
    if (p == b) die("expecting a rule name");
    return std::string(b, p);
  }
  uint32_t hex(int n) {
    uint32_t v = 0;
    for (int i = 0; i < n; i++, p++) {
      const char c = *p;
      int d;
      if (c >= '0' && c <= '9') d = c - '0';
      else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
      else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
      else die("expecting " + std::to_string(n) + " hex digits in an escape");
      v = v << 4 | (uint32_t)d;
    }
    if (v > 0x10FFFF || (v >= 0xD800 && v <= 0xDFFF)) die("escape is not a Unicode code point");
    return v;
  }
  uint32_t ch() {
    if (!*p) die("unexpected end of input");
    if (*p == '\\') {
      const char e = p[1];
      if (!e) die("unexpected end of input after a backslash");
      p += 2;
      switch (e) {
        case 'n': return '\n';
        case 'r': return '\r';
        case 't': return '\t';
        case '\\': case '"': case '[': case ']': return (uint32_t)e;
        case 'x': return hex(2);
        case 'u': return hex(4);
        case 'U': return hex(8);
        default: p -= 1; die("unknown escape");
      }
    }
    Dec d;
    uint32_t cp = 0;
    for (;;) {
      if (!*p) die("unexpected end of input inside a UTF-8 sequence");
      const int r = d.feed((uint8_t)*p, &cp);
      if (r < 0) die("the grammar text is not valid UTF-8");
      p++;
      if (r > 0) return cp;
    }
  }
  int cls_of(CharClass c) {
    normalize(c);
    g.classes.push_back(std::move(c));
    return (int)g.classes.size() - 1;
  }
  int number() {
    if (*p < '0' || *p > '9') die("expecting a number in a repetition");
    uint64_t v = 0;
    while (*p >= '0' && *p <= '9') {
      v = v * 10 + (uint64_t)(*p++ - '0');
      if (v > MAX_ELEMENTS) die("repetition count too large");
    }
    return (int)v;
  }
  // out[start..] becomes one reference to a helper rule that matches it min..max times (max < 0: no upper bound)
  void repeat(std::vector<Elem>& out, size_t start, int min, int max, const std::string& rule) {
    std::vector<Elem> item(out.begin() + start, out.end());
    out.resize(start);
    Elem x;
    if (item.size() == 1) x = item[0];
    else {
      x.ref = helper(rule);
      add_alt(x.ref, item);
    }
    std::vector<Elem> seq((size_t)min, x);
    if (max < 0) {
      Elem s;
      s.ref = helper(rule);
      add_alt(s.ref, {x, s});
      add_alt(s.ref, {});
      seq.push_back(s);
    } else if (max > min) {
      Elem prev;  // opt_k ::= x opt_(k-1) | (nothing)
      for (int k = 1; k <= max - min; k++) {
        Elem o;
        o.ref = helper(rule);
        if (k == 1) add_alt(o.ref, {x});
        else add_alt(o.ref, {x, prev});
        add_alt(o.ref, {});
        prev = o;
      }
      seq.push_back(prev);
    }
    Elem r;
    r.ref = helper(rule);
    add_alt(r.ref, std::move(seq));
    out.push_back(r);
  }
  std::vector<Elem> sequence(const std::string& rule, bool nested) {
    std::vector<Elem> out;
    size_t last = 0;
    bool have = false;
    while (*p) {
      if (*p == '"') {
        p++;
        last = out.size();
        while (*p != '"') {
          if (!*p) die("unterminated string literal", rule);
          CharClass c;
          const uint32_t v = ch();
          c.ranges.push_back({v, v});
          Elem e;
          e.cls = cls_of(c);
          out.push_back(e);
        }
        p++;
        have = true;
        if (out.size() == last) {  // "": matches nothing, as a unit that can still be repeated
          Elem e;
          e.ref = helper(rule);
          add_alt(e.ref, {});
          out.push_back(e);
        }
        space(nested);
      } else if (*p == '[') {
        p++;
        CharClass c;
        if (*p == '^') c.negated = true, p++;
        while (*p != ']') {
          if (!*p) die("unterminated character class", rule);
          const uint32_t lo = ch();
          uint32_t hi = lo;
          if (p[0] == '-' && p[1] != ']') {
            p++;
            if (!*p) die("unterminated character class", rule);
            hi = ch();
            if (hi < lo) die("character range out of order", rule);
          }
          c.ranges.push_back({lo, hi});
        }
        p++;
        last = out.size();
        Elem e;
        e.cls = cls_of(c);
        out.push_back(e);
        have = true;
        space(nested);
      } else if (*p == '.') {
        p++;
        CharClass c;
        c.negated = true;  // the complement of nothing
        last = out.size();
        Elem e;
        e.cls = cls_of(c);
        out.push_back(e);
        have = true;
        space(nested);
      } else if (*p == '(') {
        p++;
        space(true);
        Elem e;
        e.ref = helper(rule);
        alternates(e.ref, rule, true);
        if (*p != ')') die("expecting ')'", rule);
        p++;
        last = out.size();
        out.push_back(e);
        have = true;
        space(nested);
      } else if (word(*p)) {
        const std::string n = name();
        Elem e;
        e.ref = rule_id(n);
        if (first_ref[e.ref].empty()) first_ref[e.ref] = rule;
        last = out.size();
        out.push_back(e);
        have = true;
        space(nested);
        if (p[0] == ':' && p[1] == ':' && p[2] == '=') die("expecting a newline before the next rule", rule);
      } else if (*p == '*' || *p == '+' || *p == '?' || *p == '{') {
        if (!have) die("expecting an item before the repetition", rule);
        int min = 0, max = -1;
        if (*p == '*') p++;
        else if (*p == '+') min = 1, p++;
        else if (*p == '?') max = 1, p++;
        else {
          p++;
          space(nested);
          min = number();
          space(nested);
          if (*p == '}') max = min;
          else if (*p == ',') {
            p++;
            space(nested);
            if (*p != '}') {
              max = number();
              space(nested);
            }
          }
          if (*p != '}') die("expecting '}'", rule);
          if (max >= 0 && max < min)
            die("repetition {" + std::to_string(min) + "," + std::to_string(max) + "} has n < m", rule);
          p++;
        }
        repeat(out, last, min, max, rule);
        last = out.size() - 1;
        space(nested);
      } else break;
    }
    return out;
  }
  void alternates(int id, const std::string& rule, bool nested) {
    for (;;) {
      add_alt(id, sequence(rule, nested));
      if (*p != '|') break;
      p++;
      space(true);
    }
  }
  void run() {
    space(true);
    while (*p) {
      const std::string n = name();
      const int id = rule_id(n);
      if (defined[id]) die("rule '" + n + "' is defined twice");
      defined[id] = 1;
      space(false);
      if (!(p[0] == ':' && p[1] == ':' && p[2] == '=')) die("expecting '::='", n);
      p += 3;
      space(true);
      alternates(id, n, false);
      if (*p == '\r') p++;
      if (*p == '\n') p++;
      else if (*p) die("expecting a newline or the end of the grammar", n);
      space(true);
    }
    for (size_t i = 0; i < defined.size(); i++)
      if (!defined[i])
        throw ParseError{"grammar: undefined rule '" + g.rule_names[i] + "' referenced in rule '" + first_ref[i] + "'"};
    auto it = ids.find("root");
    if (it == ids.end()) throw ParseError{"grammar: no 'root' rule"};
    g.root = it->second;
  }
};

// a rule from which the rule itself can be reached without consuming a code point; -1 when there is none
int left_recursive(const Grammar& g) {
  const int n = (int)g.rules.size();
  std::vector<char> nullable(n, 0);
  for (bool changed = true; changed;) {
    changed = false;
    for (int r = 0; r < n; r++) {
      if (nullable[r]) continue;
      for (int32_t a : g.rules[r]) {
        bool all = true;
        for (const Elem& e : g.alts[a]) all &= e.ref >= 0 && nullable[e.ref];
        if (all) {
          nullable[r] = 1, changed = true;
          break;
        }
      }
    }
  }
  std::vector<std::vector<int>> edge(n);  // r -> the rules an alternative of r can begin with
  for (int r = 0; r < n; r++)
    for (int32_t a : g.rules[r])
      for (const Elem& e : g.alts[a]) {
        if (e.ref < 0) break;
        edge[r].push_back(e.ref);
        if (!nullable[e.ref]) break;
      }
  std::vector<char> color(n, 0);  // 0 new, 1 on the path, 2 done
  for (int s = 0; s < n; s++) {
    if (color[s]) continue;
    std::vector<std::pair<int, size_t>> path{{s, 0}};
    color[s] = 1;
    while (!path.empty()) {
      const int r = path.back().first;
      if (path.back().second == edge[r].size()) {
        color[r] = 2;
        path.pop_back();
        continue;
      }
      const int t = edge[r][path.back().second++];
      if (color[t] == 1) {
        // a rule of the cycle that the grammar's author wrote, if there is one
        size_t k = path.size();
        while (k-- > 0 && path[k].first != t) {}
        for (size_t i = k; i < path.size(); i++) {
          const std::string& nm = g.rule_names[path[i].first];
          const bool helper = nm.find('#') != std::string::npos;
          if (!helper) return path[i].first;
        }
        return t;
      }
      if (color[t] == 0) {
        color[t] = 1;
        path.push_back({t, 0});
      }
    }
  }
  return -1;
}
}  // namespace

std::string Grammar::create(std::shared_ptr<const Vocab> vocab, const char* text, int cache_entries,
                            std::shared_ptr<Grammar>* out) {
  if (!vocab || !text) return "grammar: null vocabulary or text";
  auto g = std::make_shared<Grammar>();
  g->vocab = std::move(vocab);
  g->cache_cap = cache_entries < 0 ? 0 : (size_t)cache_entries;
  try {
    Parser ps(*g, text);
    ps.run();
  } catch (const ParseError& e) {
    return e.msg;
  }
  const int lr = left_recursive(*g);
  if (lr >= 0) return "grammar: rule '" + g->rule_names[lr] + "' is left-recursive";
  *out = g;
  return "";
}

// ---------------------------------------------------------------- matcher

// Work is counted in stack elements touched (a stack popped from the work list, copied or compared costs its
// depth + 1); *work grows and a call gives up (false) once it passes WORK_BUDGET, as it does when a set passes
// MAX_POSITIONS.  `seen` is shared by the expansions of one set: stacks that meet again (the tail of a chain of
// nullable repetitions, reached from every stack above it) are expanded once, so a set costs what it holds.
bool Grammar::expand(const Stack& st, std::set<Stack>& seen, std::vector<Stack>& out, uint64_t* work) const {
  // a work list, without recursion (a chain of helper rules can be as long as a repetition count)
  if (!seen.insert(st).second) return true;
  std::vector<Stack> todo{st};
  while (!todo.empty()) {
    Stack s = std::move(todo.back());
    todo.pop_back();
    *work += s.size() + 1;
    if (*work > WORK_BUDGET) return false;
    if (s.empty() || alts[s.back().alt][s.back().idx].cls >= 0) {
      out.push_back(std::move(s));
      if (out.size() > MAX_POSITIONS) return false;
      continue;
    }
    const Pos top = s.back();
    const Elem& e = alts[top.alt][top.idx];
    s.pop_back();
    if ((size_t)top.idx + 1 < alts[top.alt].size()) s.push_back(Pos{top.alt, top.idx + 1});
    for (int32_t a : rules[e.ref]) {
      Stack ns = s;
      if (!alts[a].empty()) ns.push_back(Pos{a, 0});
      *work += ns.size() + 1;
      if (seen.insert(ns).second) todo.push_back(std::move(ns));
    }
  }
  return true;
}

bool Grammar::initial(std::vector<Stack>& out, uint64_t* work) const {
  out.clear();
  std::set<Stack> seen;
  for (int32_t a : rules[root]) {
    Stack s;
    if (!alts[a].empty()) s.push_back(Pos{a, 0});
    if (!expand(s, seen, out, work)) return false;
  }
  std::sort(out.begin(), out.end());  // unique already: every stack passed through `seen`
  return true;
}

bool Grammar::advance(const std::vector<Stack>& in, uint32_t c, std::vector<Stack>& out, uint64_t* work) const {
  out.clear();
  std::set<Stack> seen;
  for (const Stack& st : in) {
    *work += 1;
    if (st.empty()) continue;
    const Pos top = st.back();
    if (!classes[alts[top.alt][top.idx].cls].has(c)) continue;
    Stack ns(st.begin(), st.end() - 1);
    if ((size_t)top.idx + 1 < alts[top.alt].size()) ns.push_back(Pos{top.alt, top.idx + 1});
    if (!expand(ns, seen, out, work)) return false;
  }
  std::sort(out.begin(), out.end());
  return true;
}

bool Grammar::hits(const std::vector<Stack>& in, uint32_t lo, uint32_t hi) const {
  for (const Stack& st : in)
    if (!st.empty() && classes[alts[st.back().alt][st.back().idx].cls].hits(lo, hi)) return true;
  return false;
}

namespace {
// The walk of the vocabulary for one mask.  The stack sets it passes through are interned, and what a code point
// makes of a set is remembered, so a set is advanced once per code point however many pieces pass through it: the
// work is that of the distinct (set, code point) pairs plus one step per byte of the pieces that survive.
struct Walk {
  const Grammar& g;
  const Vocab& v;
  std::vector<uint32_t>& words;
  bool cap = false;
  uint64_t work = 0;
  std::map<std::vector<Stack>, int> ids;
  std::vector<const std::vector<Stack>*> sets;
  std::unordered_map<uint64_t, int> next_of;  // (set << 32 | code point) -> set, -1: no stack survives
  std::unordered_map<uint64_t, bool> hit_of;  // (set << 32 | first code point of the interval) -> some class hits it
  int intern(std::vector<Stack>&& s) {
    work += s.size();
    auto it = ids.emplace(std::move(s), (int)sets.size());
    if (it.second) sets.push_back(&it.first->first);
    return it.first->second;
  }
  int step(int set, uint32_t cp) {
    const uint64_t key = (uint64_t)set << 32 | cp;
    auto it = next_of.find(key);
    if (it != next_of.end()) return it->second;
    std::vector<Stack> next;
    if (!g.advance(*sets[set], cp, next, &work)) {
      cap = true;
      return -1;
    }
    const int id = next.empty() ? -1 : intern(std::move(next));
    next_of[key] = id;
    return id;
  }
  // tokens order[lo, hi) share their first `depth` bytes, which led to (set, dec)
  void run(size_t lo, size_t hi, size_t depth, int set, const Dec& dec) {
    size_t i = lo;
    for (; i < hi && v.len(v.order[i]) == depth; i++) {
      const int32_t t = v.order[i];
      words[t >> 5] |= 1u << (t & 31);
    }
    while (i < hi && !cap) {
      const uint8_t b = v.piece(v.order[i])[depth];
      size_t j = i + 1;
      while (j < hi && v.piece(v.order[j])[depth] == b) j++;
      Dec d = dec;
      uint32_t cp = 0;
      const int r = d.feed(b, &cp);
      if (++work > WORK_BUDGET) cap = true;
      if (r > 0 && !cap) {
        const int next = step(set, cp);
        if (next >= 0) run(i, j, depth + 1, next, d);
      } else if (r == 0 && !cap) {
        uint32_t clo, chi;
        Utf8::range(d.buf, d.n, &clo, &chi);
        const uint64_t key = (uint64_t)set << 32 | clo;  // a prefix is known by the first code point behind it ...
        auto it = hit_of.find(key ^ ((uint64_t)d.n << 28));  // ... and its length (U+0800 starts E0 and E0 A0)
        bool h;
        if (it != hit_of.end()) h = it->second;
        else {
          work += sets[set]->size();
          h = hit_of[key ^ ((uint64_t)d.n << 28)] = g.hits(*sets[set], clo, chi);
        }
        if (h) run(i, j, depth + 1, set, d);
      }
      i = j;
    }
  }
};

bool pending_dec(const std::string& pending, Dec* d) {
  uint32_t cp;
  for (char c : pending)
    if (d->feed((uint8_t)c, &cp) != 0) return false;
  return true;
}
}  // namespace

// words: ceil(V / 32) + 1; the last word is 1 when the walk went over the position cap (the mask is then empty)
void Grammar::compute_mask(const std::vector<Stack>& stacks, const std::string& pending,
                           std::vector<uint32_t>& words) const {
  const Vocab& v = *vocab;
  const size_t nw = ((size_t)v.n_vocab + 31) / 32;
  words.assign(nw + 1, 0u);
  Dec d;
  pending_dec(pending, &d);
  Walk w{*this, v, words};
  w.run(0, v.order.size(), 0, w.intern(std::vector<Stack>(stacks)), d);
  last_work = w.work;
  if (w.cap) {
    words.assign(nw + 1, 0u);
    words[nw] = 1;
    return;
  }
  if (pending.empty() && std::any_of(stacks.begin(), stacks.end(), [](const Stack& s) { return s.empty(); }))
    for (int32_t t : v.eog) words[t >> 5] |= 1u << (t & 31);
}

std::shared_ptr<const std::vector<uint32_t>> Grammar::mask(const std::vector<Stack>& stacks,
                                                            const std::string& pending) {
  std::string key;
  if (cache_cap) {
    for (const Stack& s : stacks) {
      const int32_t n = (int32_t)s.size();
      key.append(reinterpret_cast<const char*>(&n), 4);
      if (n) key.append(reinterpret_cast<const char*>(s.data()), (size_t)n * sizeof(Pos));
    }
    const int32_t end = -1;
    key.append(reinterpret_cast<const char*>(&end), 4);
    key += pending;
    std::lock_guard<std::mutex> lk(mu);
    auto it = index.find(key);
    if (it != index.end()) {
      n_hits++;
      lru.splice(lru.begin(), lru, it->second);
      return it->second->mask;
    }
  }
  auto m = std::make_shared<std::vector<uint32_t>>();
  compute_mask(stacks, pending, *m);
  std::lock_guard<std::mutex> lk(mu);
  n_misses++;
  if (cache_cap && !index.count(key)) {
    lru.push_front(Entry{key, m});
    index[key] = lru.begin();
    while (lru.size() > cache_cap) {
      index.erase(lru.back().key);
      lru.pop_back();
    }
  }
  return m;
}

void Grammar::stats(uint64_t* hits_, uint64_t* misses_, uint64_t* entries) {
  std::lock_guard<std::mutex> lk(mu);
  if (hits_) *hits_ = n_hits;
  if (misses_) *misses_ = n_misses;
  if (entries) *entries = lru.size();
}

// ---------------------------------------------------------------- state

State::State(std::shared_ptr<Grammar> g_) : g(std::move(g_)) {
  uint64_t work = 0;
  overflow = !g->initial(stacks, &work);
}

bool State::may_end() const {
  if (done || overflow || !pending.empty()) return false;
  return std::any_of(stacks.begin(), stacks.end(), [](const Stack& s) { return s.empty(); });
}

int State::mask(std::shared_ptr<const std::vector<uint32_t>>* out) {
  const size_t nw = ((size_t)g->vocab->n_vocab + 31) / 32;
  if (done || overflow) {
    *out = std::make_shared<std::vector<uint32_t>>(nw + 1, 0u);
    return overflow ? STATE_CAP : STATE_DEAD_END;
  }
  *out = g->mask(stacks, pending);
  const std::vector<uint32_t>& w = **out;
  if (w[nw]) return STATE_CAP;
  for (size_t i = 0; i < nw; i++)
    if (w[i]) return STATE_OK;
  return STATE_DEAD_END;
}

bool State::accept(int32_t t) {
  const Vocab& v = *g->vocab;
  if (done || overflow || t < 0 || t >= v.n_vocab) return false;
  if (v.is_eog[t]) {
    if (!may_end()) return false;
    done = true;
    return true;
  }
  const size_t n = v.len(t);
  if (!n) return false;
  Dec d;
  pending_dec(pending, &d);
  std::vector<Stack> cur = stacks, next;
  uint64_t work = 0;
  const uint8_t* b = v.piece(t);
  for (size_t i = 0; i < n; i++) {
    uint32_t cp = 0;
    const int r = d.feed(b[i], &cp);
    if (r < 0) return false;
    if (r > 0) {
      if (!g->advance(cur, cp, next, &work)) {  // over the cap: the state is lost, and the next mask says so
        overflow = true;
        stacks.clear();
        pending.clear();
        return true;
      }
      if (next.empty()) return false;
      cur.swap(next);
    }
  }
  if (d.n) {
    uint32_t lo, hi;
    Utf8::range(d.buf, d.n, &lo, &hi);
    if (!g->hits(cur, lo, hi)) return false;
  }
  stacks.swap(cur);
  pending.assign(reinterpret_cast<const char*>(d.buf), (size_t)d.n);
  return true;
}

}  // namespace gram
}  // namespace mx
