// Runs the sparse program's generator (csrc/dice_program_gen.cpp: plan_program, emit_program) under
// AddressSanitizer + UndefinedBehaviorSanitizer. No HIP, no shared library, no Python.
// Input: one binary dice_templates written by tests/test_sanitizers.py -- int32 T, int32 V, then
// lf_bits, lf_size, fields_set_size, length_slack, length, is_cc as raw arrays. Output: the source
// for the full-bitset tile and for the compact tile with the VALU and the matrix-core match stage,
// as <out>.bits, <out>.valu, <out>.mfma. Any sanitizer finding aborts the process.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dice_program_gen.h"

namespace {

std::vector<char> buf;
size_t pos = 0;

template <class T>
std::vector<T> arr(size_t n) {
    std::vector<T> v(n);
    if (pos + sizeof(T) * n > buf.size()) {
        fprintf(stderr, "input too short\n");
        exit(2);
    }
    if (n) memcpy(v.data(), buf.data() + pos, sizeof(T) * n);
    pos += sizeof(T) * n;
    return v;
}

bool write_text(const std::string& path, const std::string& text) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    return fclose(f) == 0 && ok;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        buf.resize((size_t)ftell(f));
        fseek(f, 0, SEEK_SET);
        if (fread(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
        fclose(f);
    }
    const auto hdr = arr<int32_t>(2);
    const int32_t T = hdr[0], V = hdr[1];
    if (T < 1 || V < 1) return 2;
    const auto lf = arr<uint64_t>((size_t)T * ((V + 63) / 64));
    const auto lf_size = arr<uint32_t>(T), fields = arr<uint32_t>(T);
    const auto slack = arr<int32_t>(T), length = arr<int32_t>(T);
    const auto is_cc = arr<uint8_t>(T);
    const dice_templates t{T, V, lf.data(), lf_size.data(), fields.data(), slack.data(), length.data(), is_cc.data()};

    struct Leg {
        const char* name;
        bool compact;
        dice::ProgramOptions::Match match;
    };
    const Leg legs[] = {{"bits", false, dice::ProgramOptions::kAuto},
                        {"valu", true, dice::ProgramOptions::kValu},
                        {"mfma", true, dice::ProgramOptions::kMfma}};
    size_t chars = 0;
    for (const Leg& leg : legs) {
        dice::ProgramOptions o;
        o.compact = leg.compact;
        o.match = leg.match;
        const dice::Program p = dice::plan_program(&t, o);
        const std::string src = dice::emit_program(&t, p);
        if (!write_text(std::string(argv[2]) + "." + leg.name, src)) return 3;
        chars += src.size();
    }
    printf("ok T=%d V=%d chars=%zu\n", T, V, chars);
    return 0;
}
