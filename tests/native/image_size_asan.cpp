// Stand-alone driver of the image sizing host twin for a sanitizer build (tests/test_host_image_size.py compiles this file
// together with csrc/host_image_size.cpp under -fsanitize=address,undefined and runs it as a child process; it links
// nothing else of the library, hence the error-string stub below).
//   image_size_asan <in> <out>
// <in>:  int64 n, int64 src_bytes, int64 dst_bytes, n wv_size_stage records, src_bytes bytes of images.
// <out>: the dst_bytes bytes wv_image_size_cpu wrote (0xAB where it wrote nothing).
// Source and destination live in heap blocks of exactly src_bytes / dst_bytes: one byte read or written past either end of
// the ragged batch is a sanitizer report.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "wvhash.h"

namespace wv {
static char g_err[512];
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace wv

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t head[3];
    if (fread(head, sizeof(head), 1, f) != 1) return 4;
    const int64_t n = head[0], src_bytes = head[1], dst_bytes = head[2];
    std::vector<wv_size_stage> stages((size_t)n);
    if (n && fread(stages.data(), sizeof(wv_size_stage), (size_t)n, f) != (size_t)n) return 5;
    uint8_t *src = new uint8_t[(size_t)src_bytes];
    uint8_t *dst = new uint8_t[(size_t)dst_bytes];
    if (src_bytes && fread(src, 1, (size_t)src_bytes, f) != (size_t)src_bytes) return 6;
    fclose(f);
    memset(dst, 0xAB, (size_t)dst_bytes);
    const int rc = wv_image_size_cpu(src, dst, stages.data(), (int)n);
    if (rc != WV_OK) {
        fprintf(stderr, "wv_image_size_cpu: rc = %d: %s\n", rc, wv::g_err);
        return 7;
    }
    f = fopen(argv[2], "wb");
    if (!f || (dst_bytes && fwrite(dst, 1, (size_t)dst_bytes, f) != (size_t)dst_bytes)) return 8;
    fclose(f);
    delete[] src;
    delete[] dst;
    printf("image_size_asan ok: %lld stages\n", (long long)n);
    return 0;
}
