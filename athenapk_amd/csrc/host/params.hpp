// params.hpp -- Athena-style input deck reader ("<block>" headers, "key = value" lines,
// '#' comments) with "block/key=value" command-line overrides.  Plays the role of
// Parthenon's ParameterInput for the options Hydro::Initialize reads
// (src/hydro/hydro.cpp:264-826): GetOrAdd* semantics with the same defaults, Get* throws on
// a missing key like the reference aborts.
#pragma once

#include <cstdlib>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace apk {

class ParameterInput {
 public:
  void LoadFromString(const std::string &text) {
    std::istringstream in(text);
    std::string line, block;
    while (std::getline(in, line)) {
      const auto hash = line.find('#');
      if (hash != std::string::npos) line.erase(hash);
      line = Trim(line);
      if (line.empty()) continue;
      if (line.front() == '<') {
        const auto close = line.find('>');
        if (close == std::string::npos) throw std::runtime_error("deck: unterminated block header: " + line);
        block = Trim(line.substr(1, close - 1));
        blocks_.insert(block);
        continue;
      }
      const auto eq = line.find('=');
      if (eq == std::string::npos) throw std::runtime_error("deck: expected key = value: " + line);
      if (block.empty()) throw std::runtime_error("deck: key outside of a block: " + line);
      values_[block + "/" + Trim(line.substr(0, eq))] = Trim(line.substr(eq + 1));
    }
  }
  // "block/key=value" (block may itself contain '/', e.g. parthenon/mesh/nx1=64)
  void ApplyOverride(const std::string &arg) {
    const auto eq = arg.find('=');
    if (eq == std::string::npos) throw std::runtime_error("override must be block/key=value: " + arg);
    const std::string path = Trim(arg.substr(0, eq));
    if (path.find('/') == std::string::npos) throw std::runtime_error("override must be block/key=value: " + arg);
    values_[path] = Trim(arg.substr(eq + 1));
    defaults_.erase(path);
  }
  // names of the blocks that start with `prefix` (e.g. "parthenon/output"), in deck order of
  // their names
  std::vector<std::string> BlocksWithPrefix(const std::string &prefix) const {
    std::vector<std::string> out;
    for (const auto &kv : values_) {
      const std::string block = kv.first.substr(0, kv.first.rfind('/'));
      if (block.compare(0, prefix.size(), prefix) == 0 && (out.empty() || out.back() != block)) out.push_back(block);
    }
    return out;
  }
  // a "<block>" header in the deck (keys or not), or an override into it
  bool DoesBlockExist(const std::string &block) const {
    if (blocks_.count(block)) return true;
    for (const auto &kv : values_)
      if (kv.first.size() > block.size() && kv.first.compare(0, block.size(), block) == 0 && kv.first[block.size()] == '/' &&
          kv.first.find('/', block.size() + 1) == std::string::npos)
        return true;
    return false;
  }
  // the deck as parsed with the overrides applied, every block and key, as deck text that LoadFromString reads back
  // (blocks in the order of their names; a block without keys keeps its header).  What GetOrAdd* added as a default is
  // left out: the reader adds it again, and a block that exists only through its defaults would read back as one the
  // deck has -- which some options ask about (DoesBlockExist).
  std::string Dump() const {
    std::map<std::string, std::vector<std::pair<std::string, std::string>>> by_block;
    for (const std::string &b : blocks_) by_block[b];
    for (const auto &kv : values_) {
      if (defaults_.count(kv.first)) continue;
      const auto slash = kv.first.rfind('/');
      by_block[kv.first.substr(0, slash)].emplace_back(kv.first.substr(slash + 1), kv.second);
    }
    std::string out;
    for (const auto &b : by_block) {
      out += "<" + b.first + ">\n";
      for (const auto &kv : b.second) out += kv.first + " = " + kv.second + "\n";
      out += "\n";
    }
    return out;
  }
  // the keys of one block, in the order of their names
  std::vector<std::string> KeysOf(const std::string &block) const {
    std::vector<std::string> out;
    const std::string pre = block + "/";
    for (auto it = values_.lower_bound(pre); it != values_.end() && it->first.compare(0, pre.size(), pre) == 0; ++it)
      if (it->first.find('/', pre.size()) == std::string::npos) out.push_back(it->first.substr(pre.size()));
    return out;
  }
  void Set(const std::string &block, const std::string &key, const std::string &value) {
    values_[block + "/" + key] = value;
    defaults_.erase(block + "/" + key);
  }
  void Erase(const std::string &block, const std::string &key) {
    values_.erase(block + "/" + key);
    defaults_.erase(block + "/" + key);
  }
  bool DoesParameterExist(const std::string &block, const std::string &key) const {
    return values_.count(block + "/" + key) > 0;
  }
  std::string GetString(const std::string &block, const std::string &key) const {
    auto it = values_.find(block + "/" + key);
    if (it == values_.end()) throw std::runtime_error("deck: missing required parameter <" + block + "> " + key);
    return it->second;
  }
  double GetReal(const std::string &b, const std::string &k) const { return ToReal(GetString(b, k), b, k); }
  int GetInteger(const std::string &b, const std::string &k) const { return (int)ToInt(GetString(b, k), b, k); }
  bool GetBoolean(const std::string &b, const std::string &k) const { return ToBool(GetString(b, k), b, k); }
  std::string GetOrAddString(const std::string &b, const std::string &k, const std::string &def) {
    if (!DoesParameterExist(b, k)) {
      values_[b + "/" + k] = def;
      defaults_.insert(b + "/" + k);
    }
    return GetString(b, k);
  }
  double GetOrAddReal(const std::string &b, const std::string &k, double def) {
    if (!DoesParameterExist(b, k)) {
      std::ostringstream os;
      os.precision(17);
      os << def;
      values_[b + "/" + k] = os.str();
      defaults_.insert(b + "/" + k);
      return def;
    }
    return GetReal(b, k);
  }
  int GetOrAddInteger(const std::string &b, const std::string &k, int def) {
    if (!DoesParameterExist(b, k)) {
      values_[b + "/" + k] = std::to_string(def);
      defaults_.insert(b + "/" + k);
      return def;
    }
    return GetInteger(b, k);
  }
  bool GetOrAddBoolean(const std::string &b, const std::string &k, bool def) {
    if (!DoesParameterExist(b, k)) {
      values_[b + "/" + k] = def ? "true" : "false";
      defaults_.insert(b + "/" + k);
      return def;
    }
    return GetBoolean(b, k);
  }

 private:
  static std::string Trim(const std::string &s) {
    const char *ws = " \t\r\n";
    const auto a = s.find_first_not_of(ws);
    if (a == std::string::npos) return "";
    const auto b = s.find_last_not_of(ws);
    return s.substr(a, b - a + 1);
  }
  static double ToReal(const std::string &v, const std::string &b, const std::string &k) {
    char *end = nullptr;
    const double x = std::strtod(v.c_str(), &end);
    if (end == v.c_str()) throw std::runtime_error("deck: <" + b + "> " + k + " is not a number: " + v);
    return x;
  }
  static long ToInt(const std::string &v, const std::string &b, const std::string &k) {
    char *end = nullptr;
    const long x = std::strtol(v.c_str(), &end, 10);
    if (end == v.c_str()) throw std::runtime_error("deck: <" + b + "> " + k + " is not an integer: " + v);
    return x;
  }
  static bool ToBool(const std::string &v, const std::string &b, const std::string &k) {
    if (v == "true" || v == "True" || v == "1") return true;
    if (v == "false" || v == "False" || v == "0") return false;
    throw std::runtime_error("deck: <" + b + "> " + k + " is not a boolean: " + v);
  }
  std::map<std::string, std::string> values_;
  std::set<std::string> blocks_;  // block headers seen in the deck
  std::set<std::string> defaults_;  // block/key of the values GetOrAdd* added (not the deck's, not an override's)
};

}  // namespace apk
