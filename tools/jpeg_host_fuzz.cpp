// Stand-alone driver for the host half of the JPEG decoder (csrc/jpeg.hip: dbn_jpeg_info_ex, dbn_jpeg_coef_elems_ex,
// dbn_jpeg_entropy_batch_ex), meant to be built with host sanitizers; it never touches a GPU.  Every stream is copied into a
// heap block of exactly its length and decoded into a coefficient block of exactly the size asked for, with and without the
// multiscan flag, so that a read or write one byte outside either is a sanitizer report.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I db_text_minimal_amd/csrc db_text_minimal_amd/csrc/jpeg.hip tools/jpeg_host_fuzz.cpp -o jpeg_host_fuzz
//   ./jpeg_host_fuzz streams.bin      streams.bin: int32 count, then per stream int32 length and the bytes
// (tests/test_jpeg_scans_cpu.py's truncations and corruptions of tests/golden/jpeg_scans_cases.npz are a good input.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" {
int dbn_jpeg_info_ex(const unsigned char* data, long len, int flags, long long* out);
long dbn_jpeg_coef_elems_ex(const unsigned char* blob, const long long* offs, int N, int flags, long long* per_image);
int dbn_jpeg_entropy_batch_ex(const unsigned char* blob, const long long* offs, int N, short* coef, long coef_elems, long long* desc,
                              unsigned short* qtabs, int* status, int* orientation, int threads, int flags);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    long by_status[2][16] = {};
    for (int i = 0; i < count; ++i) {
        int len = 0;
        if (fread(&len, 4, 1, f) != 1 || len < 0) return 2;
        unsigned char* d = (unsigned char*)malloc(len ? len : 1);
        if (len && fread(d, 1, len, f) != (size_t)len) return 2;
        if (!len) {  // an empty stream still needs a pointer: one byte that is never read
            free(d);
            d = (unsigned char*)malloc(1);
        }
        for (int flags = 0; flags < 2; ++flags) {
            long long info[24], offs[2] = {0, len}, per = 0, desc[24];
            if (dbn_jpeg_info_ex(d, len, flags, info) != 0) return 3;
            const long total = dbn_jpeg_coef_elems_ex(d, offs, 1, flags, &per);
            if (total < 0 || total != per || total != info[15]) return 3;
            short* coef = (short*)malloc(total ? total * sizeof(short) : 1);
            unsigned short qt[192];
            int status = -1, orientation = -1;
            if (dbn_jpeg_entropy_batch_ex(d, offs, 1, coef, total, desc, qt, &status, &orientation, 1, flags) != 0) return 3;
            if (status < 0 || status > 14 || orientation < 0 || orientation > 8) return 3;
            ++by_status[flags][status];
            free(coef);
        }
        free(d);
    }
    for (int flags = 0; flags < 2; ++flags) {
        printf("flags %d:", flags);
        for (int s = 0; s < 15; ++s) printf(" %d:%ld", s, by_status[flags][s]);
        printf("\n");
    }
    return 0;
}
