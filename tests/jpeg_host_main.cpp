// The JPEG decoder's arithmetic (stmask_amd/csrc/jpeg_core.h) run on the CPU over a batch that stmask_amd.jpeg.pack_batch laid out: the same
// descriptors, tables and segments the gfx950 kernels read, the same functions per symbol, block and pixel, in plain loops.  A stand-alone
// program, so that tests/test_jpeg_cpu.py can build it with -fsanitize=address,undefined and run it on sound and on damaged files.
//
//   jpeg_host_main JOB     JOB: int64 [8] n_images, n_segments, images_off, segments_off, blob_bytes, out_bytes, bgr, 0 | the blob | the expected
//                          frames (out_bytes, laid out as the decoder's out) | int32 [n_images] lenient
// Prints one line per image: "<i> equal", "<i> flagged <status>" or "<i> differs".  A strict image must be equal; a lenient one (a damaged file)
// must be flagged or equal.  Exit status 0 when every image keeps to that, 1 otherwise, 2 for a job the argument checks refuse.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../stmask_amd/csrc/jpeg_core.h"

namespace {

struct HostSource {
    const uint8_t* seg;
    int get(int pos) { return seg[pos]; }
};

struct HostSink {
    int16_t* blk;
    void put(int k, int v) { blk[jpeg_natural(k)] = (int16_t)v; }
};

bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[8];
    if (!read_all(f, h, sizeof(h))) return 2;
    const int n_images = (int)h[0], n_segments = (int)h[1];
    const size_t images_off = (size_t)h[2], segments_off = (size_t)h[3], blob_bytes = (size_t)h[4], out_bytes = (size_t)h[5];
    const int bgr = (int)h[6];
    std::vector<uint8_t> blob(blob_bytes), want(out_bytes), out(out_bytes, 0xAA);
    std::vector<int32_t> lenient((size_t)n_images);
    if (!read_all(f, blob.data(), blob_bytes) || !read_all(f, want.data(), out_bytes) || !read_all(f, lenient.data(), 4 * (size_t)n_images)) return 2;
    fclose(f);
    if (images_off + (size_t)n_images * sizeof(stm_jpeg_image) > blob_bytes || segments_off + (size_t)n_segments * sizeof(stm_jpeg_segment) > blob_bytes) return 2;
    std::vector<stm_jpeg_image> images((size_t)n_images);
    std::vector<stm_jpeg_segment> segments((size_t)n_segments);
    memcpy(images.data(), blob.data() + images_off, images.size() * sizeof(stm_jpeg_image));
    memcpy(segments.data(), blob.data() + segments_off, segments.size() * sizeof(stm_jpeg_segment));
    int64_t total_blocks = 0, total_quads = 0;
    const char* why = "";
    int which = 0;
    if (jpeg_check_batch(images.data(), n_images, segments.data(), n_segments, blob_bytes, out_bytes, &total_blocks, &total_quads, &why, &which) != STM_OK) {
        printf("refused: image or segment %d has %s\n", which, why);
        return 2;
    }
    std::vector<int16_t> coef((size_t)total_blocks * 64, 0);
    std::vector<uint8_t> planes((size_t)total_blocks * 64, 0);
    std::vector<int> status((size_t)n_segments, 0);

    // launch 1: one segment after the other
    for (int s = 0; s < n_segments; ++s) {
        const stm_jpeg_segment& sg = segments[s];
        const stm_jpeg_image& im = images[sg.image];
        stm_jpeg_tables tables;
        memcpy(&tables, blob.data() + im.src_off, sizeof(tables));
        // the segment alone in a buffer of its own size: a read past it is a read out of bounds
        std::vector<uint8_t> bytes(blob.begin() + sg.byte_off, blob.begin() + sg.byte_off + sg.nbytes);
        HostSource src{bytes.data()};
        JpegBits<HostSource> br(src, sg.nbytes);
        int pred[3] = {0, 0, 0};
        int err = 0;
        for (int m = 0; m < sg.mcu_count && !err; ++m) {
            const int mcu = sg.mcu_first + m, my = mcu / im.mcu_w, mx = mcu % im.mcu_w;
            for (int c = 0; c < im.ncomp && !err; ++c) {
                const int hs = jpeg_comp_hs(im, c), vs = jpeg_comp_vs(im, c), bw = im.mcu_w * hs;
                for (int by = 0; by < vs && !err; ++by)
                    for (int bx = 0; bx < hs && !err; ++bx) {
                        const int64_t blk = (int64_t)im.blk_first + jpeg_comp_first(im, c) + (int64_t)(my * vs + by) * bw + (mx * hs + bx);
                        HostSink sink{coef.data() + blk * 64};
                        const JpegHuffRef dc{&tables.huff[im.td[c]]}, ac{&tables.huff[2 + im.ta[c]]};
                        err = jpeg_decode_block(br, dc, ac, pred[c], sink);
                        if (err) memset(sink.blk, 0, 128);
                    }
            }
        }
        status[s] = err;
    }
    // launch 2: every block
    for (int i = 0; i < n_images; ++i) {
        const stm_jpeg_image& im = images[i];
        if (im.kind != STM_JPEG_DECODE) continue;
        stm_jpeg_tables tables;
        memcpy(&tables, blob.data() + im.src_off, sizeof(tables));
        for (int c = 0; c < im.ncomp; ++c) {
            const int bw = jpeg_comp_bw(im, c), bh = jpeg_comp_bh(im, c);
            const int64_t first = (int64_t)im.blk_first + jpeg_comp_first(im, c);
            for (int b = 0; b < bw * bh; ++b) {
                int32_t tile[8][8], in[8], o[8];
                for (int k = 0; k < 64; ++k) tile[k >> 3][k & 7] = (int32_t)coef[(first + b) * 64 + k] * (int32_t)tables.quant[im.tq[c]][k];
                for (int j = 0; j < 8; ++j) {
                    for (int r = 0; r < 8; ++r) in[r] = tile[r][j];
                    jpeg_idct8(in, o, 11);
                    for (int r = 0; r < 8; ++r) tile[r][j] = o[r];
                }
                const int by = b / bw, bx = b % bw;
                for (int j = 0; j < 8; ++j) {
                    jpeg_idct8(tile[j], o, 18);
                    for (int r = 0; r < 8; ++r) planes[(size_t)first * 64 + ((size_t)(by * 8 + j) * bw + bx) * 8 + r] = (uint8_t)jpeg_sample(o[r]);
                }
            }
        }
    }
    // launch 3: every pixel
    int bad = 0;
    for (int i = 0; i < n_images; ++i) {
        const stm_jpeg_image& im = images[i];
        const size_t n = (size_t)im.width * im.height;
        uint8_t* dst = out.data() + im.out_off;
        if (im.kind == STM_JPEG_RAW) {
            memcpy(dst, blob.data() + im.src_off, 3 * n);
        } else {
            for (int y = 0; y < im.height; ++y)
                for (int x = 0; x < im.width; ++x) {
                    int r, g, b;
                    jpeg_pixel(im, planes.data() + (size_t)64 * im.blk_first, x, y, r, g, b);
                    uint8_t* p = dst + 3 * ((size_t)y * im.width + x);
                    p[0] = (uint8_t)(bgr ? b : r);
                    p[1] = (uint8_t)g;
                    p[2] = (uint8_t)(bgr ? r : b);
                }
        }
        int st = 0;
        for (int s = 0; s < n_segments && !st; ++s)
            if (segments[s].image == i) st = status[s];
        const bool equal = memcmp(dst, want.data() + im.out_off, 3 * n) == 0;
        if (st) printf("%d flagged %d\n", i, st);
        else printf("%d %s\n", i, equal ? "equal" : "differs");
        if (st ? !lenient[i] : !equal) bad = 1;
    }
    return bad;
}
