// The split entropy decode (stmask_amd/csrc/jpeg_split_core.h) run on the CPU over a batch that stmask_amd.jpeg.pack_batch(split=...) laid out:
// the functions the gfx950 kernels of csrc/jpeg_split.hip call per lane, with the kernels' grouping, round count, record layout and parities in
// plain loops, then the serial decode of the segments marked REDO, the IDCT and the colour conversion as tests/jpeg_host_main.cpp has them.  A
// stand-alone program, so that tests/test_jpeg_split_cpu.py can build it with -fsanitize=address,undefined and run it on sound and on damaged
// files; it is the model of which segments converge.
//
//   jpeg_split_host_main JOB [FRAMES]    JOB: as tests/jpeg_host_main.cpp reads it (tests/jpeg_cases.py write_job); FRAMES: a file to write the
//                                        decoded frames to (out_bytes, laid out as the decoder's out), to compare two runs' pixels
// Prints one line per image: "<i> equal|differs|flagged <status> split|serial|redone" -- serial: the image was not split; redone: it was, and
// the serial decode ran after all; the status is the serial path's, without STM_JPEG_REDONE.  Exit status as jpeg_host_main's.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../stmask_amd/csrc/jpeg_split_core.h"

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

constexpr int GROUP = STM_JPEG_SUB_GROUP, ROUNDS = STM_JPEG_SPLIT_ROUNDS;

// one launch of jpeg_split_sync_kernel over the groups of one image
void sync_round(HostSource& src, int nbytes, const stm_jpeg_huff* huff, int n0, int bpm, int tsel, JpegSplitRec* rec, int round)
{
    const int n_sub = jpeg_split_subs(nbytes), par = round & 1;
    const bool last = round == ROUNDS;
    JpegSplitNull none;
    for (int sub0 = 0; sub0 < n_sub; sub0 += GROUP) {
        uint32_t e[GROUP] = {0}, x[GROUP] = {0}, x_was[GROUP] = {0}, s_x[GROUP];
        const int lanes = n_sub - sub0 < GROUP ? n_sub - sub0 : GROUP;
        for (int lane = 0; lane < lanes; ++lane) {
            const int sub = sub0 + lane;
            if (round == 0) {
                e[lane] = sub == 0 ? 0u : jpeg_split_guess(src, nbytes, sub);
                x[lane] = jpeg_split_run(src, nbytes, huff, n0, bpm, tsel, sub, e[lane], none);
            } else {
                const uint32_t e_was = rec[sub].e[par ^ 1];
                x[lane] = x_was[lane] = rec[sub].x[par ^ 1];
                e[lane] = sub == 0 ? 0u : rec[sub - 1].x[par ^ 1];
                if (e[lane] != e_was) x[lane] = jpeg_split_run(src, nbytes, huff, n0, bpm, tsel, sub, e[lane], none);
            }
        }
        for (int it = 0; it < GROUP; ++it) {
            bool any = false;
            memcpy(s_x, x, sizeof(x));
            for (int lane = 1; lane < lanes; ++lane)
                if (s_x[lane - 1] != e[lane]) {
                    e[lane] = s_x[lane - 1];
                    x[lane] = jpeg_split_run(src, nbytes, huff, n0, bpm, tsel, sub0 + lane, e[lane], none);
                    any = true;
                }
            if (!any) break;
        }
        for (int lane = 0; lane < lanes; ++lane) {
            const int sub = sub0 + lane;
            rec[sub].e[par] = e[lane];
            rec[sub].x[par] = x[lane];
            if (round == 0 && sub == 0) rec[0].redo = 0;
            if (last) {
                if (x[lane] != x_was[lane]) rec[0].redo = 1;
                JpegSplitCount cnt = {0, 0, 0, 0};
                jpeg_split_run(src, nbytes, huff, n0, bpm, tsel, sub, e[lane], cnt);
                rec[sub].blocks = cnt.blocks;
                rec[sub].dc[0] = (int16_t)cnt.d0;
                rec[sub].dc[1] = (int16_t)cnt.d1;
                rec[sub].dc[2] = (int16_t)cnt.d2;
            }
        }
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2 && argc != 3) return 2;
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
    // the planes as 32-byte records where the split launches use them so (two per block: never more than the image's region, jpeg_split_fits)
    std::vector<JpegSplitRec> plane_words((size_t)total_blocks * 2 + 1);
    memset(plane_words.data(), 0xAA, plane_words.size() * sizeof(JpegSplitRec));
    uint8_t* planes = reinterpret_cast<uint8_t*>(plane_words.data());
    std::vector<int> status((size_t)n_segments, 0), redo((size_t)n_images, 0);

    // the split launches, image by image
    for (int s = 0; s < n_segments; ++s) {
        const stm_jpeg_segment& sg = segments[s];
        const stm_jpeg_image& im = images[sg.image];
        if (!(im.split & 1)) continue;
        stm_jpeg_tables tables;
        memcpy(&tables, blob.data() + im.src_off, sizeof(tables));
        std::vector<uint8_t> bytes(blob.begin() + sg.byte_off, blob.begin() + sg.byte_off + sg.nbytes);      // alone: a read past it is out of bounds
        HostSource src{bytes.data()};
        const int n0 = im.hs * im.vs, bpm = jpeg_blocks_per_mcu(im), tsel = jpeg_split_tables(im), n_sub = jpeg_split_subs(sg.nbytes);
        // the records alone as well: n_sub of them
        std::vector<JpegSplitRec> recs((size_t)n_sub);
        memset(recs.data(), 0xAA, recs.size() * sizeof(JpegSplitRec));
        JpegSplitRec* rec = recs.data();
        for (int round = 0; round <= ROUNDS; ++round) sync_round(src, sg.nbytes, tables.huff, n0, bpm, tsel, rec, round);
        // scan
        unsigned carry[4] = {0, 0, 0, 0};
        for (int i = 0; i < n_sub; ++i) {
            const unsigned v[4] = {(unsigned)rec[i].blocks, (unsigned)rec[i].dc[0], (unsigned)rec[i].dc[1], (unsigned)rec[i].dc[2]};
            rec[i].blocks = (int)carry[0];
            for (int q = 0; q < 3; ++q) rec[i].dc[q] = (int16_t)carry[1 + q];
            for (int q = 0; q < 4; ++q) carry[q] += v[q];
        }
        if ((int)carry[0] < 0 || (int64_t)(int)carry[0] < (int64_t)sg.mcu_count * bpm) rec[0].redo = 1;
        // write
        const int par = ROUNDS & 1;
        for (int sub = 0; sub < n_sub && !rec[0].redo; ++sub) {
            JpegSplitWrite w;
            w.coef = coef.data();
            w.first = im.blk_first;
            w.hs = im.hs;
            w.vs = im.vs;
            w.mcu_w = im.mcu_w;
            w.mcu_h = im.mcu_h;
            w.mcu_first = 0;
            w.n0 = n0;
            w.bpm = bpm;
            w.expected = im.mcu_w * im.mcu_h * bpm;
            w.seq = rec[sub].blocks;
            w.preds = (uint64_t)(uint16_t)rec[sub].dc[0] | ((uint64_t)(uint16_t)rec[sub].dc[1] << 16) | ((uint64_t)(uint16_t)rec[sub].dc[2] << 32);
            w.bad = 0;
            const uint32_t e = rec[sub].e[par];
            const JpegSplitState st = jpeg_split_unpack(e, sub * STM_JPEG_SUB_BYTES, bpm);
            w.open(st.k ? w.seq - 1 : -1, st.u);
            jpeg_split_run(src, sg.nbytes, tables.huff, n0, bpm, tsel, sub, e, w);
            if (w.bad) recs[0].redo = 1;        // (the kernel's lanes all run; a later lane's stores do not matter once the mark is set)
        }
        redo[sg.image] = rec[0].redo;
        // the records had their place in the planes: show that they fit there
        if ((size_t)n_sub * sizeof(JpegSplitRec) > (size_t)64 * jpeg_image_blocks(im)) return 2;
        memcpy(planes + (size_t)64 * im.blk_first, rec, (size_t)n_sub * sizeof(JpegSplitRec));
    }
    // launch 1: one segment after the other; of a split image only when marked
    for (int s = 0; s < n_segments; ++s) {
        const stm_jpeg_segment& sg = segments[s];
        const stm_jpeg_image& im = images[sg.image];
        int redone = 0;
        if (im.split & 1) {
            if (!redo[sg.image]) {
                status[s] = 0;
                continue;
            }
            redone = STM_JPEG_REDONE;
            memset(coef.data() + (size_t)64 * im.blk_first, 0, (size_t)128 * jpeg_image_blocks(im));     // (the kernel stores every block whole)
        }
        stm_jpeg_tables tables;
        memcpy(&tables, blob.data() + im.src_off, sizeof(tables));
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
        status[s] = err | redone;
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
                    jpeg_pixel(im, planes + (size_t)64 * im.blk_first, x, y, r, g, b);
                    uint8_t* p = dst + 3 * ((size_t)y * im.width + x);
                    p[0] = (uint8_t)(bgr ? b : r);
                    p[1] = (uint8_t)g;
                    p[2] = (uint8_t)(bgr ? r : b);
                }
        }
        int st = 0;
        for (int s = 0; s < n_segments && !st; ++s)
            if (segments[s].image == i) st = status[s] & ~STM_JPEG_REDONE;
        const bool equal = memcmp(dst, want.data() + im.out_off, 3 * n) == 0;
        const char* mode = !(im.split & 1) ? "serial" : (redo[i] ? "redone" : "split");
        if (st) printf("%d flagged %d %s\n", i, st, mode);
        else printf("%d %s %s\n", i, equal ? "equal" : "differs", mode);
        if (st ? !lenient[i] : !equal) bad = 1;
    }
    if (argc == 3) {
        FILE* g = fopen(argv[2], "wb");
        if (!g || fwrite(out.data(), 1, out.size(), g) != out.size() || fclose(g) != 0) return 2;
    }
    return bad;
}
