// gguf.h -- minimal GGUF v2/v3 parser (mmap) for the engine's model loader.
// Replaces the GGUF parse inside Llama(model_path=...) (/root/reference/llama_p2p_network.py:19;
// SURVEY.md §8a row a2).
#pragma once
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

namespace mx {

struct GGUFValue {
  int type = -1;  // GGUF value type
  double num = 0;
  std::string str;
  std::vector<double> arr_num;
  std::vector<std::string> arr_str;
  int arr_type = -1;
};

struct GGUFTensor {
  std::string name;
  std::vector<uint64_t> ne;  // ne[0] fastest
  int type = 0;              // ggml type
  uint64_t offset = 0;       // absolute file offset
  uint64_t nbytes = 0;
};

class GGUFFile {
 public:
  ~GGUFFile();
  // returns empty string on success, else an error message
  std::string open(const std::string& path);
  const GGUFValue* get(const std::string& key) const;
  double get_num(const std::string& key, double dflt) const;
  const GGUFTensor* tensor(const std::string& name) const;
  const uint8_t* data(const GGUFTensor& t) const { return base_ + t.offset; }
  std::map<std::string, GGUFValue> kv;
  std::map<std::string, GGUFTensor> tensors;
  uint64_t file_size = 0;

 private:
  uint8_t* base_ = nullptr;
  int fd_ = -1;
};

// A GGUF LoRA adapter (convert_lora_to_gguf.py) checked against its base model.  For a base tensor
// T of ne = {n_in, n_out}: T.lora_a of ne = {n_in, r}, row-major A[r][n_in], and T.lora_b of ne = {r, n_out},
// row-major B[n_out][r]; W' = W + scale * B A.
struct LoraPair {
  const GGUFTensor* a = nullptr;
  const GGUFTensor* b = nullptr;
  int layer = 0;  // the N of blk.N.*
  int r = 0;      // lora_b.ne[0]
  int n_in = 0, n_out = 0;
};
struct LoraAdapter {
  GGUFFile file;
  float alpha = 0.f;                      // adapter.lora.alpha
  std::map<std::string, LoraPair> pairs;  // by base tensor name
  // opens `path` and checks it against `base`: general.type / adapter.type / architecture, every .lora_a with its
  // .lora_b, F32 / F16 / BF16 only, shapes against the base tensor, r >= 1, and only the seven layer matrices
  // blk.N.{attn_q,attn_k,attn_v,attn_output,ffn_gate,ffn_up,ffn_down}.weight as targets.  Returns an empty string,
  // else the reason with the offending tensor or key named.
  std::string open(const std::string& path, const GGUFFile& base);
  // llama.cpp's llama_lora_weight::get_scale: lora_scale * alpha / r, or lora_scale alone when alpha is 0
  float scale(const LoraPair& p, float lora_scale) const {
    return alpha != 0.f ? lora_scale * alpha / (float)p.r : lora_scale;
  }
  // an adapter tensor (F32 / F16 / BF16) as f32, n = its element count
  void to_f32(const GGUFTensor& t, float* dst) const;
};

}  // namespace mx
