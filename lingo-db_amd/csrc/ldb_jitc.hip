// ldb_jitc <source file> <arch> <code object out> <log out> — one hiprtc compilation of a specialised translation unit in a process of its own
// (hiprtc serialises the compilations inside one process; see compile_in_child in ldb_jit.hip).  No device is used.
// Exit status: 0 = code object written, 1 = hiprtc refused the unit (log written), anything else = the helper itself failed.
#include "ldb_jit_compile.h"

int main(int argc, char** argv) {
   if (argc != 5) return 2;
   std::string src, err;
   if (FILE* f = fopen(argv[1], "rb")) {
      char buf[65536];
      for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) src.append(buf, n);
      fclose(f);
   }
   std::vector<char> code;
   if (src.empty()) return 3;
   if (!compile(src, &code, &err, argv[2])) { // exit status 1 = the compiler's own verdict, its log in argv[4]
      if (FILE* f = fopen(argv[4], "wb")) {
         fwrite(err.data(), 1, err.size(), f);
         fclose(f);
      }
      return 1;
   }
   FILE* f = fopen(argv[3], "wb");
   bool ok = f && fwrite(code.data(), 1, code.size(), f) == code.size();
   if (f) ok = fclose(f) == 0 && ok;
   return ok ? 0 : 3;
}
