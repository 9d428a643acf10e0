// tests/_hostsim/jpegdec_corrupt_main.cpp -- TEST INFRASTRUCTURE ONLY.
// A stand-alone program over a set of corrupt JPEG files (tests/test_jpegdec_cpu.py writes the set: truncations and single-byte corruptions of a small file), for
// a build with -fsanitize=address,undefined: every case goes through the host build of csrc/y7t_jpegdec.h with a workspace and a frame of exactly the sizes the
// ABI asks for, so a read or write one byte outside either ends the program.  The set: int32 n, then per case int32 H, W, sampling, subseq_bytes, lanes, file_len,
// the 80-byte record and the file's bytes.  Prints how many cases it ran and how many reported a status.
#include "y7t_hostsim_jpegdec.cpp"
#include <stdio.h>
#include <stdlib.h>

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <set>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int n = 0, flagged = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    for (int i = 0; i < n; ++i) {
        int h[6];
        Y7TJdDesc d;
        if (fread(h, 4, 6, f) != 6 || fread(&d, sizeof(d), 1, f) != 1) return 2;
        std::vector<unsigned char> file((size_t)h[5]);
        if (h[5] && fread(file.data(), 1, file.size(), f) != file.size()) return 2;
        const size_t ws_bytes = hs_jpegdec_bytes(h[0], h[1], h[2], d.file_len, h[3], h[4]);
        if (!ws_bytes) return 3;
        unsigned char* ws = (unsigned char*)calloc(ws_bytes, 1);
        unsigned char* frame = (unsigned char*)malloc((size_t)h[0] * h[1] * 3);
        int info[5] = {0, 0, 0, 0, 0};
        const int rc = hs_jpegdec_decode(file.data(), &d, h[0], h[1], h[2], h[3], h[4], ws, nullptr, nullptr, frame, info);
        if (rc == 0 && info[0]) ++flagged;
        free(frame);
        free(ws);
    }
    fclose(f);
    printf("%d cases, %d with a status\n", n, flagged);
    return 0;
}
