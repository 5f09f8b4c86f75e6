// ldb_strfn.h — device helpers shared by the string-valued computed columns (ldb_expr.hip: substr; ldb_strfn.hip:
// concatenation, case mapping, length).  Ahead-of-time kernels only: not one of the sources hiprtc compiles.
#pragma once
#include "ldb_device.h"

// StringRuntime::substr(str, from, len) (reference src/runtime/StringRuntime.cpp:292-319): positions
// count UTF-8 CHARACTERS from 1; positions before the string "count towards the length"; from / to
// beyond the end are truncated to it (charIndexToByteIndex, :102-135).
__device__ __forceinline__ uint32_t d_char_to_byte(const uint8_t* s, uint32_t byte_len, uint64_t char_index, uint32_t known_byte, uint64_t known_char) {
   for (; known_byte < byte_len; known_byte++) {
      if ((s[known_byte] >> 6) != 2) { // not a continuation byte
         if (known_char == char_index) return known_byte;
         known_char++;
      }
   }
   return byte_len;
}
__device__ __forceinline__ void d_substr_range(const uint8_t* s, uint32_t len, int64_t from, int64_t for_len, uint32_t* b0, uint32_t* b1) {
   const int64_t leg_len = for_len > 0 ? for_len : 0;
   uint64_t leg_from = (uint64_t) (from > 1 ? from : 1);
   const int64_t to_raw = from + leg_len;
   uint64_t leg_to = to_raw > (int64_t) leg_from ? (uint64_t) to_raw : leg_from;
   leg_from--;
   leg_to--;
   *b0 = d_char_to_byte(s, len, leg_from, 0, 0);
   *b1 = d_char_to_byte(s, len, leg_to, *b0, leg_from);
}
