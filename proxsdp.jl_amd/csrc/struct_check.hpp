// The ABI guard of the model handle's structs (include/proxsdp_hip.h): a struct whose struct_size is not this library's sizeof
// was laid out by another ABI version and is refused before a field of it is believed.  No HIP in this file: the *_host.hpp
// halves use it, and they build with a plain C++17 compiler.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

namespace proxsdp {

// q: not NULL; name: the struct's, as the message spells it
template <typename T>
inline void check_struct_size(const T* q, const char* name) {
    if (q->struct_size != (int64_t)sizeof(T)) throw std::invalid_argument(std::string(name) + ".struct_size mismatch");
}

}  // namespace proxsdp
