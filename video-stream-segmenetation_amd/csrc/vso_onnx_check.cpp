// vso_onnx_check.cpp — a stand-alone driver for the model reader and the
// constant folding (vso_onnx.cpp, vso_fold.cpp), built with AddressSanitizer
// and UBSan by `make onnx-asan`: the code that takes a user's file, run on
// the host without a GPU.  For each path given it parses the file and folds
// every node whose inputs are all constants, as session creation would, and
// prints one tab-separated line:
//   ok <TAB> opset=.. <TAB> nodes=.. <TAB> inits=.. <TAB> folded=.. <TAB> inputs=a,b <TAB> outputs=c,d
//   error <TAB> <message>
// Exit status 0 unless a file cannot be read; a sanitizer report aborts.
#include <cstdio>
#include <fstream>
#include <iterator>

#include "vso_onnx.h"

using namespace vso_onnx;

namespace {

// folds the graph's constant nodes in order; the number folded, or -1 with *err set
int fold_constants(const Graph& g, std::string* err) {
  std::map<std::string, Const> consts = g.inits;
  int folded = 0;
  for (const Node& nd : g.nodes) {
    std::vector<Operand> in;
    bool all_const = true;
    for (const std::string& n : nd.in) {
      auto it = n.empty() ? consts.end() : consts.find(n);
      if (it != consts.end()) in.push_back(Operand{&it->second.dims, &it->second});
      else in.push_back(Operand{});
      all_const = all_const && (n.empty() || it != consts.end());
    }
    if (nd.op != "Constant" && (!all_const || in.empty() || nd.op == "Conv")) continue;
    if (nd.out.empty()) { *err = "node '" + nd.name + "' has no output"; return -1; }
    Const r;
    if (!fold(nd, in, &r, err)) return -1;
    consts[nd.out[0]] = r;
    ++folded;
  }
  return folded;
}

std::string names(const std::vector<IO>& v) {
  std::string s;
  for (const IO& io : v) s += (s.empty() ? "" : ",") + io.name;
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  for (int k = 1; k < argc; ++k) {
    std::ifstream f(argv[k], std::ios::binary);
    if (!f) {
      std::fprintf(stderr, "cannot read %s\n", argv[k]);
      return 2;
    }
    const std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    Graph g;
    std::string err;
    int folded = -1;
    if (parse_model(bytes.data(), bytes.size(), &g, &err)) folded = fold_constants(g, &err);
    if (folded < 0)
      std::printf("error\t%s\n", err.c_str());
    else
      std::printf("ok\topset=%lld\tnodes=%zu\tinits=%zu\tfolded=%d\tinputs=%s\toutputs=%s\n", (long long)g.opset,
                  g.nodes.size(), g.inits.size(), folded, names(g.inputs).c_str(), names(g.outputs).c_str());
  }
  return 0;
}
