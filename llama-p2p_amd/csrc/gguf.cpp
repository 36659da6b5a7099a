// gguf.cpp -- GGUF v2/v3 container parser (header, typed metadata, tensor
// infos, aligned data section), read through mmap so multi-GB models are
// never copied into host RAM before upload.
#include "gguf.h"

#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <stdexcept>

namespace mx {

namespace {
enum { T_UINT8, T_INT8, T_UINT16, T_INT16, T_UINT32, T_INT32, T_FLOAT32, T_BOOL, T_STRING, T_ARRAY, T_UINT64,
       T_INT64, T_FLOAT64 };

struct Cursor {
  const uint8_t* p;
  const uint8_t* end;
  void need(uint64_t n) {
    if ((uint64_t)(end - p) < n) throw std::runtime_error("GGUF: truncated file");
  }
  template <class T>
  T rd() {
    need(sizeof(T));
    T v;
    memcpy(&v, p, sizeof(T));
    p += sizeof(T);
    return v;
  }
  std::string str() {
    uint64_t n = rd<uint64_t>();
    need(n);
    std::string s((const char*)p, n);
    p += n;
    return s;
  }
};

double scalar(Cursor& c, int t) {
  switch (t) {
    case T_UINT8: return c.rd<uint8_t>();
    case T_INT8: return c.rd<int8_t>();
    case T_UINT16: return c.rd<uint16_t>();
    case T_INT16: return c.rd<int16_t>();
    case T_UINT32: return c.rd<uint32_t>();
    case T_INT32: return c.rd<int32_t>();
    case T_FLOAT32: return c.rd<float>();
    case T_BOOL: return c.rd<uint8_t>() ? 1.0 : 0.0;
    case T_UINT64: return (double)c.rd<uint64_t>();
    case T_INT64: return (double)c.rd<int64_t>();
    case T_FLOAT64: return c.rd<double>();
  }
  throw std::runtime_error("GGUF: bad scalar type " + std::to_string(t));
}

// bytes of n elements of a ggml type (n < 2^56 checked by the caller, so nothing here overflows);
// 0 for an unsupported type or a count that is not a whole number of blocks
uint64_t type_bytes(int type, uint64_t n) {
  uint64_t blk = 1, bb = 0;
  switch (type) {
    case 0: bb = 4; break;                   // F32
    case 1: bb = 2; break;                   // F16
    case 30: bb = 2; break;                  // BF16
    case 8: blk = 32, bb = 34; break;        // Q8_0
    case 2: blk = 32, bb = 18; break;        // Q4_0
    case 12: blk = 256, bb = 144; break;     // Q4_K
    case 13: blk = 256, bb = 176; break;     // Q5_K
    case 14: blk = 256, bb = 210; break;     // Q6_K
    default: return 0;
  }
  if (n % blk) return 0;
  return n / blk * bb;
}
}  // namespace

GGUFFile::~GGUFFile() {
  if (base_) munmap(base_, file_size);
  if (fd_ >= 0) close(fd_);
}

std::string GGUFFile::open(const std::string& path) {
  fd_ = ::open(path.c_str(), O_RDONLY);
  if (fd_ < 0) return "cannot open " + path;
  struct stat st;
  if (fstat(fd_, &st) != 0) return "cannot stat " + path;
  file_size = (uint64_t)st.st_size;
  if (file_size < 24) return path + ": file too small for GGUF";
  void* m = mmap(nullptr, file_size, PROT_READ, MAP_SHARED, fd_, 0);
  if (m == MAP_FAILED) return "mmap failed for " + path;
  base_ = (uint8_t*)m;
  try {
    Cursor c{base_, base_ + file_size};
    if (memcmp(c.p, "GGUF", 4) != 0) return path + ": bad magic (not a GGUF file)";
    c.p += 4;
    uint32_t version = c.rd<uint32_t>();
    if (version != 2 && version != 3) return "unsupported GGUF version " + std::to_string(version);
    uint64_t n_t = c.rd<uint64_t>(), n_kv = c.rd<uint64_t>();
    for (uint64_t i = 0; i < n_kv; i++) {
      std::string key = c.str();
      GGUFValue v;
      v.type = (int)c.rd<uint32_t>();
      if (v.type == T_STRING) {
        v.str = c.str();
      } else if (v.type == T_ARRAY) {
        v.arr_type = (int)c.rd<uint32_t>();
        uint64_t n = c.rd<uint64_t>();
        // every element takes at least 1 byte (8 for a string's length): a count beyond what the
        // file holds is truncation, reported before any allocation of that size
        const uint64_t left = (uint64_t)(c.end - c.p);
        if (n > (v.arr_type == T_STRING ? left / 8 : left)) throw std::runtime_error("GGUF: truncated array " + key);
        if (v.arr_type == T_STRING) {
          v.arr_str.reserve(n);
          for (uint64_t j = 0; j < n; j++) v.arr_str.push_back(c.str());
        } else {
          v.arr_num.reserve(n);
          for (uint64_t j = 0; j < n; j++) v.arr_num.push_back(scalar(c, v.arr_type));
        }
      } else {
        v.num = scalar(c, v.type);
      }
      kv[key] = std::move(v);
    }
    std::vector<GGUFTensor> infos;
    for (uint64_t i = 0; i < n_t; i++) {
      GGUFTensor t;
      t.name = c.str();
      uint32_t nd = c.rd<uint32_t>();
      if (nd > 4) return "GGUF: tensor with >4 dims";
      uint64_t n = 1;
      for (uint32_t d = 0; d < nd; d++) {
        t.ne.push_back(c.rd<uint64_t>());
        if (__builtin_mul_overflow(n, t.ne.back(), &n) || n >= (1ull << 56))
          return "GGUF: tensor " + t.name + " has an element count that overflows";
      }
      t.type = (int)c.rd<uint32_t>();
      t.offset = c.rd<uint64_t>();
      t.nbytes = type_bytes(t.type, n);
      if (t.nbytes == 0 && n != 0)
        return "GGUF: tensor " + t.name + " has unsupported type " + std::to_string(t.type) +
               " (or a ragged block count)";
      infos.push_back(t);
    }
    const double al_num = get_num("general.alignment", 32);
    if (!(al_num >= 1 && al_num <= 65536)) return "GGUF: general.alignment out of range";
    const uint64_t al = (uint64_t)al_num;
    if (al & (al - 1)) return "GGUF: general.alignment " + std::to_string(al) + " is not a power of two";
    const uint64_t hdr = (uint64_t)(c.p - base_);
    const uint64_t data_start = (hdr + al - 1) / al * al;
    if (data_start > file_size) return "GGUF: data section starts past end of file";
    for (auto& t : infos) {
      // offset and size are checked against the bytes after data_start without forming sums that wrap
      const uint64_t room = file_size - data_start;
      if (t.offset > room || t.nbytes > room - t.offset)
        return "GGUF: tensor " + t.name + " extends past end of file";
      t.offset += data_start;
      tensors[t.name] = t;
    }
  } catch (const std::exception& e) {
    return e.what();
  }
  return "";
}

const GGUFValue* GGUFFile::get(const std::string& key) const {
  auto it = kv.find(key);
  return it == kv.end() ? nullptr : &it->second;
}

double GGUFFile::get_num(const std::string& key, double dflt) const {
  const GGUFValue* v = get(key);
  if (!v || v->type == T_STRING || v->type == T_ARRAY) return dflt;
  return v->num;
}

const GGUFTensor* GGUFFile::tensor(const std::string& name) const {
  auto it = tensors.find(name);
  return it == tensors.end() ? nullptr : &it->second;
}

namespace {
// blk.N.<one of the seven layer matrices>.weight -> N, else -1
int lora_target_layer(const std::string& name) {
  static const char* kinds[] = {"attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down"};
  if (name.rfind("blk.", 0) != 0) return -1;
  const size_t dot = name.find('.', 4);
  if (dot == std::string::npos || dot == 4 || dot > 4 + 6) return -1;
  int layer = 0;
  for (size_t i = 4; i < dot; i++) {
    if (name[i] < '0' || name[i] > '9') return -1;
    layer = layer * 10 + (name[i] - '0');
  }
  const std::string rest = name.substr(dot + 1);
  for (const char* k : kinds)
    if (rest == std::string(k) + ".weight") return layer;
  return -1;
}
bool ends_with(const std::string& s, const char* suf) {
  const size_t n = strlen(suf);
  return s.size() > n && s.compare(s.size() - n, n, suf) == 0;
}
}  // namespace

std::string LoraAdapter::open(const std::string& path, const GGUFFile& base) {
  const std::string err = file.open(path);
  if (!err.empty()) return err;
  const auto str = [&](const char* key) {
    const GGUFValue* v = file.get(key);
    return v && v->type == T_STRING ? v->str : std::string();
  };
  if (str("general.type") != "adapter") return "LoRA adapter: general.type must be 'adapter', got '" + str("general.type") + "'";
  if (str("adapter.type") != "lora") return "LoRA adapter: adapter.type must be 'lora', got '" + str("adapter.type") + "'";
  {  // the adapter's architecture is the base model's
    const GGUFValue* ba = base.get("general.architecture");
    const std::string want = ba && ba->type == T_STRING ? ba->str : std::string();
    if (str("general.architecture") != want)
      return "LoRA adapter: general.architecture must be the base model's '" + want + "', got '" +
             str("general.architecture") + "'";
  }
  alpha = (float)file.get_num("adapter.lora.alpha", 0.0);
  if (!(alpha == alpha) || alpha - alpha != 0.f) return "LoRA adapter: adapter.lora.alpha is not finite";
  pairs.clear();
  for (const auto& kvp : file.tensors) {
    const GGUFTensor& t = kvp.second;
    const bool is_a = ends_with(t.name, ".lora_a"), is_b = ends_with(t.name, ".lora_b");
    if (!is_a && !is_b) return "LoRA adapter: tensor " + t.name + " is neither a .lora_a nor a .lora_b";
    if (t.type != 0 && t.type != 1 && t.type != 30)
      return "LoRA adapter: tensor " + t.name + " has ggml type " + std::to_string(t.type) +
             " (F32, F16 and BF16 adapters are supported, quantised ones are not)";
    const std::string target = t.name.substr(0, t.name.size() - 7);
    if (!file.tensor(target + (is_a ? ".lora_b" : ".lora_a")))
      return "LoRA adapter: tensor " + t.name + " has no " + target + (is_a ? ".lora_b" : ".lora_a");
    if (!is_a) continue;  // the pair is checked once, at its .lora_a
    const GGUFTensor& b = *file.tensor(target + ".lora_b");
    const int layer = lora_target_layer(target);
    if (layer < 0)
      return "LoRA adapter: target " + target +
             " is not supported (blk.N.{attn_q,attn_k,attn_v,attn_output,ffn_gate,ffn_up,ffn_down}.weight are)";
    const GGUFTensor* w = base.tensor(target);
    if (!w) return "LoRA adapter: target " + target + " is not a tensor of the base model";
    if (w->ne.size() != 2 || t.ne.size() != 2 || b.ne.size() != 2)
      return "LoRA adapter: " + target + ": the base tensor, .lora_a and .lora_b must have two dimensions";
    if (b.ne[0] < 1 || t.ne[1] < 1) return "LoRA adapter: " + target + " has rank 0";
    if (t.ne[0] != w->ne[0]) return "LoRA adapter: " + t.name + " ne[0] does not match " + target + " ne[0]";
    if (b.ne[1] != w->ne[1]) return "LoRA adapter: " + b.name + " ne[1] does not match " + target + " ne[1]";
    if (t.ne[1] != b.ne[0]) return "LoRA adapter: " + t.name + " ne[1] and " + b.name + " ne[0] (the rank) differ";
    if (b.ne[0] > (1u << 16) || w->ne[0] > (1u << 30) || w->ne[1] > (1u << 30))
      return "LoRA adapter: " + target + " is too large";
    LoraPair p;
    p.a = &t;
    p.b = &b;
    p.layer = layer;
    p.r = (int)b.ne[0];
    p.n_in = (int)w->ne[0];
    p.n_out = (int)w->ne[1];
    pairs[target] = p;
  }
  return "";
}

void LoraAdapter::to_f32(const GGUFTensor& t, float* dst) const {
  uint64_t n = 1;
  for (uint64_t d : t.ne) n *= d;
  const uint8_t* src = file.data(t);
  if (t.type == 0) {
    memcpy(dst, src, n * 4);
  } else if (t.type == 1) {
    for (uint64_t i = 0; i < n; i++) {
      _Float16 h;
      memcpy(&h, src + 2 * i, 2);
      dst[i] = (float)h;
    }
  } else {  // BF16
    for (uint64_t i = 0; i < n; i++) {
      uint16_t h;
      memcpy(&h, src + 2 * i, 2);
      const uint32_t u = (uint32_t)h << 16;
      memcpy(dst + i, &u, 4);
    }
  }
}

}  // namespace mx
