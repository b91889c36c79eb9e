// tools/end_mask_emulate.cpp -- the end mask of pss-bam -K (pss-bam_amd/csrc/end_mask_kernels.h) compiled for the host: the
// per-record function is the kernel's own code, and the loop around it is select_mask_ends' -- a scanned dst[] with an entry per
// input record, dropped records (dst[r] == dst[r + 1]) between the kept ones.
//
//     g++ -O1 -I pss-bam_amd/csrc -o end_mask_emulate tools/end_mask_emulate.cpp && ./end_mask_emulate in.raw out.raw ds 5 5
//
// in.raw holds BAM records back to back (le32 block_size + body: what the record sink delivers); out.raw receives the masked
// stream (what the sink delivers with the mask on, which tests/test_gpu_end_mask.py checks on a device);
// tests/test_end_mask_host.py runs it where there is no GPU.  The stream lives in a heap block of exactly its size, so that built
// with -fsanitize=address,undefined a write outside it, or a read, is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "end_mask_kernels.h"

int main(int argc, char **argv) {
    if (argc != 6) { fprintf(stderr, "usage: end_mask_emulate in.raw out.raw all|ds|ss n5 n3\n"); return 2; }
    const uint32_t mode = !strcmp(argv[3], "all") ? PSSBAM_EM_ALL : !strcmp(argv[3], "ds") ? PSSBAM_EM_DS : !strcmp(argv[3], "ss") ? PSSBAM_EM_SS : PSSBAM_EM_OFF;
    const unsigned long n5 = strtoul(argv[4], nullptr, 10), n3 = strtoul(argv[5], nullptr, 10);
    if (mode == PSSBAM_EM_OFF || n5 > PSSBAM_EM_MAX_N || n3 > PSSBAM_EM_MAX_N) { fprintf(stderr, "end_mask_emulate: bad mode or width\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { fprintf(stderr, "end_mask_emulate: cannot open %s\n", argv[1]); return 1; }
    std::vector<uint8_t> raw;
    uint8_t buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, in)) > 0;) raw.insert(raw.end(), buf, buf + n);
    fclose(in);
    // dst[] as the scan leaves it: every kept record, and behind every third one a record that was dropped
    std::vector<uint32_t> dst;
    size_t at = 0;
    for (uint32_t r = 0; at < raw.size(); r++) {
        if (raw.size() - at < 4) { fprintf(stderr, "end_mask_emulate: %zu stray bytes at the end\n", raw.size() - at); return 1; }
        const uint64_t len = 4ull + pssbam_em_u32(raw.data() + at);
        if (len > raw.size() - at) { fprintf(stderr, "end_mask_emulate: record %u leaves the stream\n", r); return 1; }
        dst.push_back((uint32_t)at);
        if (r % 3u == 1u) dst.push_back((uint32_t)(at + len));   // (the dropped record's entry: where the next kept one starts)
        at += (size_t)len;
    }
    dst.push_back((uint32_t)at);
    const uint32_t n = (uint32_t)dst.size() - 1u;
    uint8_t *out = (uint8_t *)malloc(raw.size() ? raw.size() : 1);   // exactly the stream: no slack for a stray byte
    if (!out) return 1;
    memcpy(out, raw.data(), raw.size());
    for (uint32_t r = 0; r < n; r++) {   // select_mask_ends, a lane after the other
        const uint32_t d0 = dst[r], d1 = dst[r + 1u];
        if (d1 <= d0 || d1 > raw.size()) continue;
        pssbam_end_mask_record(out + d0, d1 - d0, mode, (uint32_t)n5, (uint32_t)n3);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o || fwrite(out, 1, raw.size(), o) != raw.size()) { fprintf(stderr, "end_mask_emulate: cannot write %s\n", argv[2]); return 1; }
    free(out);
    return fclose(o) ? 1 : 0;
}
