// grammar_selfcheck -- csrc/grammar.cpp alone, for a host sanitizer build:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tools/grammar_selfcheck.cpp llama-p2p_amd/csrc/grammar.cpp -o grammar_selfcheck     (one command)
//   python tests/test_grammar_host.py DIR && ./grammar_selfcheck DIR
//
// For every vocabulary (*.vocab) and grammar (*.gbnf) of DIR: compile, take seeded random walks of up to 64
// accepted tokens with and without the mask cache, and print a hash of all the masks seen (the two must agree);
// then the texts GBNF refuses, a dead end, the position cap, and a grammar destroyed while a state uses it.
// Exit status 0 when everything held.
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <string>

#include "../llama-p2p_amd/csrc/grammar.h"

using namespace mx::gram;

static int failures = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      failures++;                                              \
    }                                                          \
  } while (0)

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static std::shared_ptr<const Vocab> load_vocab(const std::string& path) {
  const std::string raw = slurp(path);
  uint32_t n = 0, ne = 0;
  if (raw.size() < 12 || memcmp(raw.data(), "MXGV", 4)) return nullptr;
  memcpy(&n, raw.data() + 4, 4);
  memcpy(&ne, raw.data() + 8, 4);
  if (raw.size() < 12 + 4 * (size_t)ne + 8 * ((size_t)n + 1)) return nullptr;
  std::vector<int32_t> eog(ne);
  std::vector<uint64_t> off((size_t)n + 1);
  memcpy(eog.data(), raw.data() + 12, 4 * (size_t)ne);
  memcpy(off.data(), raw.data() + 12 + 4 * (size_t)ne, 8 * ((size_t)n + 1));
  const size_t blob = 12 + 4 * (size_t)ne + 8 * ((size_t)n + 1);
  if (raw.size() != blob + off[n]) return nullptr;
  std::shared_ptr<const Vocab> v;
  const std::string err = Vocab::create((int)n, reinterpret_cast<const uint8_t*>(raw.data()) + blob, off.data(),
                                        eog.data(), (int)ne, &v);
  if (!err.empty()) printf("%s: %s\n", path.c_str(), err.c_str());
  return v;
}

static uint64_t walk(const std::shared_ptr<Grammar>& g, uint32_t seed) {
  uint64_t h = 1469598103934665603ull;
  const int V = g->vocab->n_vocab;
  std::mt19937 rng(seed);
  State st(g);
  for (int step = 0; step < 64; step++) {
    std::shared_ptr<const std::vector<uint32_t>> m;
    const int status = st.mask(&m);
    std::vector<int32_t> ids;
    for (int t = 0; t < V; t++)
      if (((*m)[t >> 5] >> (t & 31)) & 1u) ids.push_back(t);
    for (size_t i = 0; i < ((size_t)V + 31) / 32; i++) h = (h ^ (*m)[i]) * 1099511628211ull;
    h = (h ^ (uint64_t)status) * 1099511628211ull;
    CHECK((status == STATE_OK) == !ids.empty());
    if (ids.empty()) break;
    const int32_t t = ids[rng() % ids.size()];
    CHECK(st.accept(t));
    if (st.ended()) break;
  }
  return h;
}

int main(int argc, char** argv) {
  if (argc != 2) return printf("usage: %s DIR\n", argv[0]), 2;
  const std::string dir = argv[1];
  std::vector<std::string> vocabs, grammars;
  if (DIR* d = opendir(dir.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string n = e->d_name;
      if (n.size() > 6 && n.substr(n.size() - 6) == ".vocab") vocabs.push_back(n);
      if (n.size() > 5 && n.substr(n.size() - 5) == ".gbnf") grammars.push_back(n);
    }
    closedir(d);
  }
  std::sort(vocabs.begin(), vocabs.end());
  std::sort(grammars.begin(), grammars.end());
  if (vocabs.empty() || grammars.empty()) return printf("no *.vocab / *.gbnf in %s\n", dir.c_str()), 2;
  std::shared_ptr<const Vocab> any;
  for (const std::string& vn : vocabs) {
    std::shared_ptr<const Vocab> v = load_vocab(dir + "/" + vn);
    CHECK(v != nullptr);
    if (!v) continue;
    any = v;
    for (const std::string& gn : grammars) {
      const std::string text = slurp(dir + "/" + gn);
      std::shared_ptr<Grammar> g, g0;
      const std::string e1 = Grammar::create(v, text.c_str(), 256, &g), e0 = Grammar::create(v, text.c_str(), 0, &g0);
      CHECK(e1.empty() && e0.empty());
      if (!g || !g0) {
        printf("%s: %s\n", gn.c_str(), e1.c_str());
        continue;
      }
      for (uint32_t seed = 0; seed < 4; seed++) {
        const uint64_t a = walk(g, seed), b = walk(g0, seed), c = walk(g, seed);
        CHECK(a == b && a == c);
        printf("%-12s %-16s seed %u masks %016llx\n", vn.c_str(), gn.c_str(), seed, (unsigned long long)a);
      }
      uint64_t hits = 0, misses = 0, entries = 0;
      g->stats(&hits, &misses, &entries);
      CHECK(hits > 0 && entries <= 256);
    }
  }
  if (any) {
    const char* bad[] = {"root \"a\"\n", "root ::= \"abc\n", "root ::= [abc\n", "root ::= (\"a\" | \"b\"\n",
                         "root ::= \"a\")\n", "root ::= \"\\q\"\n", "root ::= \"\\x4\"", "root ::= \"\\", "root ::= [a-",
                         "root ::= * \"a\"\n", "root ::= \"a\"{x}\n", "root ::= \"a\"{2,3\n", "root ::= \"a\"{3,2}\n",
                         "root ::= \"a\"{99999999999}\n", "root ::= item\n", "start ::= \"a\"\n", "root ::= root \"a\"\n",
                         "root ::= a\na ::= b\nb ::= (a \"x\")?\n", "root ::= \"\xff\"\n", "::= \"a\"\n", "",
                         "root ::= \"a\"{100000}\n"};
    for (const char* t : bad) {
      std::shared_ptr<Grammar> g;
      const std::string err = Grammar::create(any, t, 4, &g);
      CHECK(!err.empty() && !g);
    }
    std::shared_ptr<Grammar> g;
    CHECK(Grammar::create(any, "root ::= s\ns ::= \"a\" s \"b\" | \"a\" s \"c\" | \"a\"\n", 4, &g).empty());
    if (g) {
      State st(g);
      int status = STATE_OK, a = -1;
      for (int t = 0; t < any->n_vocab; t++)
        if (any->len(t) == 1 && any->piece(t)[0] == 'a') a = t;
      for (int n = 0; n < 20 && status == STATE_OK && a >= 0; n++) {
        std::shared_ptr<const std::vector<uint32_t>> m;
        status = st.mask(&m);
        if (status == STATE_OK) CHECK(st.accept(a));
      }
      CHECK(status == STATE_CAP);
      std::unique_ptr<State> keep(new State(g));
      g.reset();  // the state keeps the grammar, the grammar its vocabulary
      std::shared_ptr<const std::vector<uint32_t>> m;
      CHECK(keep->mask(&m) == STATE_OK);
    }
    CHECK(Grammar::create(any, "root ::= (\"a\"?){0,10000} \".\"\n", 4, &g).empty());
    if (g) {
      std::shared_ptr<const std::vector<uint32_t>> m;
      CHECK(State(g).mask(&m) == STATE_CAP);
    }
  }
  printf(failures ? "%d checks FAILED\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
