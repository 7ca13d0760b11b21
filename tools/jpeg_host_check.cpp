// Stand-alone exerciser of the host JPEG decoder (vit-search_amd/csrc/jpeg_host.cpp), meant to be built with
// -fsanitize=address,undefined (make -C vit-search_amd/csrc jpeg_host_check) and run on files given on the command line:
//     ../build/jpeg_host_check a.jpg b.jpg ...
// For every file it runs vr_jpeg_probe / vr_jpeg_entropy_decode over the file itself, over every truncation of it, and over
// single-byte corruptions of it (every byte of the first 1024 and a stride over the rest, three replacement values each).  The
// stream and the coefficient buffer are heap blocks of exactly the sizes handed to the library, so a read or write one byte out of
// bounds is a sanitizer report.  Exit status 0: no call crashed and the intact file decoded as the probe promised.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/vitres_jpeg.h"

namespace {

struct Counts {
    long calls = 0, ok = 0, unsupported = 0, damaged = 0;
};

// one probe + decode of exactly `n` bytes in their own allocation; returns the decode's code
int run(const uint8_t* bytes, size_t n, Counts& k) {
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);
    memcpy(data, bytes, n);
    vr_jpeg_info info, info2;
    if (vr_jpeg_probe(data, (int64_t)n, &info) != 0) abort();
    int64_t total = 0;
    for (int c = 0; c < 3; ++c) total += 64 * (int64_t)info.blocks[c];
    if (!info.supported && total != 0) abort();
    int16_t* coef = (int16_t*)calloc((size_t)(total ? total : 1), sizeof(int16_t));
    uint16_t qtab[3 * 64];
    const int rc = vr_jpeg_entropy_decode(data, (int64_t)n, &info2, coef, total, qtab);
    ++k.calls;
    if (rc == 0) {
        ++k.ok;
        if (!info.supported || memcmp(&info, &info2, sizeof(info)) != 0) abort();
    } else if (rc == -3) {
        ++k.unsupported;
        if (info.supported) abort();
    } else if (rc == -1) {
        ++k.damaged;
    } else {
        abort();
    }
    free(coef);
    free(data);
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
        return 2;
    }
    Counts all;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> buf;
        uint8_t chunk[65536];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
        fclose(f);
        Counts k;
        const int whole = run(buf.data(), buf.size(), k);
        for (size_t cut = 0; cut < buf.size(); ++cut) run(buf.data(), cut, k);
        const size_t stride = buf.size() > 1024 ? (buf.size() - 1024) / 512 + 1 : 1;
        std::vector<uint8_t> bad(buf);
        for (size_t i = 0; i < buf.size(); i += (i < 1024 ? 1 : stride)) {
            const uint8_t values[3] = {(uint8_t)(buf[i] ^ 0xFF), 0xFF, (uint8_t)(buf[i] + 1)};
            for (int v = 0; v < 3; ++v) {
                bad[i] = values[v];
                run(bad.data(), bad.size(), k);
            }
            bad[i] = buf[i];
        }
        printf("%s: %zu bytes, whole file -> %d; %ld calls: %ld decoded, %ld unsupported, %ld damaged\n", argv[a], buf.size(), whole,
               k.calls, k.ok, k.unsupported, k.damaged);
        all.calls += k.calls;
        all.ok += k.ok;
        all.unsupported += k.unsupported;
        all.damaged += k.damaged;
    }
    printf("total: %ld calls: %ld decoded, %ld unsupported, %ld damaged; no sanitizer report\n", all.calls, all.ok, all.unsupported,
           all.damaged);
    return 0;
}
