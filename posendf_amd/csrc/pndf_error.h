// The error channel of every handle family of the C ABI (pndf_*_last_error): a failed call leaves its text on the handle; a
// refusal without a handle (a failed create) leaves it in a slot of the calling thread, one slot per handle type.  No HIP here:
// pndf_cpu.cpp is compiled without a device pass.
#pragma once
#include <string>

// host helpers shared by the translation units stay out of the library's dynamic symbol table: the exports are the C ABI
#define PNDF_LOCAL __attribute__((visibility("hidden")))

template <class H>
PNDF_LOCAL inline std::string& pndf_null_handle_error() {
    static thread_local std::string slot;
    return slot;
}

// records `msg` and returns `code`; without a handle name the family: pndf_fail<pndf_engine>(nullptr, ...)
template <class H>
PNDF_LOCAL inline int pndf_fail(H* h, int code, const std::string& msg) {
    (h ? h->err : pndf_null_handle_error<H>()) = msg;
    return code;
}

template <class H>
PNDF_LOCAL inline const char* pndf_last_error_of(H* h) {
    return (h ? h->err : pndf_null_handle_error<H>()).c_str();
}
