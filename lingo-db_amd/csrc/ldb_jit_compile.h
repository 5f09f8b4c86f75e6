// The run-time specialiser's compiler: the kernel headers embedded at build time and one hiprtc compilation of a specialised translation unit.
// Included by ldb_jit.hip (the library: compile on a worker thread) and by ldb_jitc.hip (the compiler process the workers start).
#pragma once
#include <hip/hiprtc.h>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

struct EmbeddedHeader {
   const char* name;
   const char* text;
};
static const EmbeddedHeader g_headers[] = {
#include "ldb_jit_sources.inc"
};
static const int g_n_headers = (int) (sizeof(g_headers) / sizeof(g_headers[0]));

// compile only (no device needed); code object into *code
static bool compile(const std::string& src, std::vector<char>* code, std::string* err, const char* arch = "gfx950") {
   std::vector<const char*> names, texts;
   for (int i = 0; i < g_n_headers; i++) {
      names.push_back(g_headers[i].name);
      texts.push_back(g_headers[i].text);
   }
   hiprtcProgram prog;
   if (hiprtcCreateProgram(&prog, src.c_str(), "ldb_spec.hip", g_n_headers, texts.data(), names.data()) != HIPRTC_SUCCESS) {
      *err = "hiprtcCreateProgram failed";
      return false;
   }
   std::vector<std::string> extra; // tuning experiments: LDB_JIT_DEFINES="-DGB_ROWS=8 -DGB_PRED_BATCH=0"
   if (const char* defs = getenv("LDB_JIT_DEFINES")) {
      std::string s(defs), tok;
      for (size_t i = 0; i <= s.size(); i++) {
         if (i == s.size() || s[i] == ' ') {
            if (!tok.empty()) extra.push_back(tok);
            tok.clear();
         } else {
            tok += s[i];
         }
      }
   }
   // The descriptor loops (LDB_UNROLL) must unroll completely or nothing folds: before unrolling
   // their bodies hold the whole generic interpreter, which exceeds the default pragma-unroll
   // size limit and silently leaves a generic loop reading the constexpr descriptor from memory.
   const std::string arch_opt = std::string("--offload-arch=") + arch;
   std::vector<const char*> opts = {arch_opt.c_str(), "-O3", "-std=c++17", "-munsafe-fp-atomics", "-mllvm", "-pragma-unroll-threshold=4000000"};
   for (auto& e : extra) opts.push_back(e.c_str());
   hiprtcResult r = hiprtcCompileProgram(prog, (int) opts.size(), opts.data());
   if (r != HIPRTC_SUCCESS) {
      size_t ls = 0;
      hiprtcGetProgramLogSize(prog, &ls);
      std::string log(ls, '\0');
      if (ls) hiprtcGetProgramLog(prog, log.data());
      *err = std::string("hiprtc: ") + hiprtcGetErrorString(r) + ": " + log.substr(0, 3000);
      hiprtcDestroyProgram(&prog);
      return false;
   }
   size_t cs = 0;
   hiprtcGetCodeSize(prog, &cs);
   code->resize(cs);
   hiprtcGetCode(prog, code->data());
   hiprtcDestroyProgram(&prog);
   if (const char* dir = getenv("LDB_JIT_DUMP_ALL")) { // every code object, numbered (offline ISA / register-usage inspection)
      static std::atomic<int> seq{0}; // (compilations run on several worker threads)
      char path[512];
      snprintf(path, sizeof(path), "%s/ldb_spec_%03d.co", dir, seq.fetch_add(1));
      if (FILE* f = fopen(path, "wb")) {
         fwrite(code->data(), 1, code->size(), f);
         fclose(f);
      }
   }
   return cs > 0;
}

