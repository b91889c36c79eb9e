// tools/deflate_emulate.cpp -- the device deflate's encoder (pss-bam_amd/csrc/deflate_kernels.h) compiled for the host: with
// DFL_EMULATE a phase of the workgroup is a loop over its threads, everything else is the kernel's own code.
//
//     g++ -O1 -I pss-bam_amd/csrc -o deflate_emulate tools/deflate_emulate.cpp && ./deflate_emulate in.raw out.bgzf
//
// cuts in.raw every 0xFF00 bytes and writes the BGZF blocks back to back (what bgzf_deflate + bgzf_pack give on a device, which
// tests/test_gpu_deflate.py checks there); tests/test_deflate_emulated_host.py runs it where there is no GPU.  Built with
// -fsanitize=address,undefined it checks the encoder's indexing on the CPU.
#define DFL_EMULATE
#include <cstdio>
#include <cstring>
#include <vector>

#include "deflate_kernels.h"

using namespace pssbam;

static uint32_t gf2_mul_host(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 0; i < 32; i++) {
        if (b & 0x80000000u) r ^= a;
        b <<= 1;
        a = (a >> 1) ^ ((a & 1u) ? DFL_CRC_POLY : 0u);
    }
    return r;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: deflate_emulate in.raw out.bgzf\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { fprintf(stderr, "deflate_emulate: cannot open %s\n", argv[1]); return 1; }
    std::vector<uint8_t> raw;
    uint8_t buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, in)) > 0;) raw.insert(raw.end(), buf, buf + n);
    fclose(in);
    static uint32_t xpow64[DFL_THREADS];   // x^(8 * 64 * k) mod P, as bgzf_api.h's ensure_xpow64
    uint32_t x64 = 0x80000000u;
    for (uint32_t i = 0; i < 8 * DFL_CRC_CHUNK; i++) x64 = (x64 >> 1) ^ ((x64 & 1u) ? DFL_CRC_POLY : 0u);
    xpow64[0] = 0x80000000u;
    for (uint32_t k = 1; k < DFL_THREADS; k++) xpow64[k] = gf2_mul_host(xpow64[k - 1], x64);
    FILE *out = fopen(argv[2], "wb");
    if (!out) { fprintf(stderr, "deflate_emulate: cannot create %s\n", argv[2]); return 1; }
    static DeflateShared S;
    alignas(16) static uint8_t payload[DFL_SLOT + 16], block[DFL_SLOT];
    for (size_t at = 0; at < raw.size(); at += DFL_PAYLOAD) {
        const uint32_t n = (uint32_t)(raw.size() - at < DFL_PAYLOAD ? raw.size() - at : DFL_PAYLOAD);
        memset(payload, 0xA5, sizeof payload);   // (what lies behind the payload must not show)
        memcpy(payload, raw.data() + at, n);
        uint32_t len = 0;
        deflate_block(S, payload, n, block, &len, xpow64);
        if (len > DFL_SLOT || fwrite(block, 1, len, out) != len) { fprintf(stderr, "deflate_emulate: block of %u bytes\n", len); return 1; }
    }
    return fclose(out) ? 1 : 0;
}
