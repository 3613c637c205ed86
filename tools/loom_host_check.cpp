// loom_host_check.cpp -- vcy_loom_block_host (csrc/ingest.hip) under the host sanitizers, as a program of its own: CPU only, no Python.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         velocyto.py_amd/csrc/ingest.hip tools/loom_host_check.cpp -o /tmp/loom_host_check -lz && /tmp/loom_host_check
//
// It writes a file of chunks it deflates itself (a (G, C) dataset in ch_r x ch_c chunks, edge chunks stored full size, one chunk never
// written, per-chunk filter masks), answers the two HDF5 calls from its own table, and compares every block with the array the chunks were
// cut from: element sizes 1 / 2 / 4 / 8, filters none / deflate / shuffle + deflate, blocks that start and end inside chunks, 1 and 4
// threads; then a truncated stream, which must come back as -4 with the chunk's number.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <vector>
#include <zlib.h>

#include "../include/velocyto_hip.h"

namespace vcy { thread_local char g_err[512]; }                          // the library's error text lives in another translation unit
extern "C" const char *vcy_last_error(void) { return vcy::g_err; }

struct Entry { uint64_t addr, size; unsigned mask; };
static std::vector<Entry> g_table;
static int64_t g_ncc, g_chr, g_chc;

static int g_fd;
static const Entry &entry(const uint64_t *at) { return g_table[(at[0] / g_chr) * g_ncc + at[1] / g_chc]; }
static int chunk_size(int64_t, const uint64_t *at, uint64_t *size)                       // stands in for H5Dget_chunk_storage_size
{
    *size = entry(at).size;
    return entry(at).addr == ~0ull ? -1 : 0;
}
static int read_chunk(int64_t, int64_t, const uint64_t *at, uint32_t *mask, void *buf)   // stands in for H5Dread_chunk
{
    const Entry &e = entry(at);
    *mask = e.mask;
    return pread(g_fd, buf, e.size, (off_t)e.addr) == (ssize_t)e.size ? 0 : -1;
}

static int run(int esz, int filters, int64_t G, int64_t C, int64_t chr, int64_t chc, bool truncate)
{
    std::vector<uint8_t> full((size_t)G * C * esz);
    uint32_t x = 12345u + esz * 7 + filters;
    for (auto &b : full) { x = x * 1664525u + 1013904223u; b = (x >> 24) < 40 ? (uint8_t)(x >> 16) : 0; }
    g_chr = chr; g_chc = chc;
    const int64_t ncr = (G + chr - 1) / chr;
    g_ncc = (C + chc - 1) / chc;
    g_table.assign(ncr * g_ncc, Entry{~0ull, 0, 0});
    char path[] = "/tmp/loom_host_check_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) return 1;
    unlink(path);
    g_fd = fd;
    const size_t raw = (size_t)chr * chc * esz;
    uint64_t off = 512;                                                   // something in front of the first chunk
    for (int64_t r = 0; r < ncr; ++r)
        for (int64_t c = 0; c < g_ncc; ++c) {
            Entry &e = g_table[r * g_ncc + c];
            if (r == 1 && c == 1) {                                       // never written: must read as zeros
                for (int64_t g = r * chr; g < G && g < (r + 1) * chr; ++g)
                    for (int64_t k = c * chc; k < C && k < (c + 1) * chc; ++k) memset(&full[((size_t)g * C + k) * esz], 0, esz);
                continue;
            }
            std::vector<uint8_t> plain(raw, 0), shuf(raw), z(compressBound(raw));
            for (int64_t g = r * chr; g < G && g < (r + 1) * chr; ++g)
                for (int64_t k = c * chc; k < C && k < (c + 1) * chc; ++k)
                    memcpy(&plain[((size_t)(g - r * chr) * chc + (k - c * chc)) * esz], &full[((size_t)g * C + k) * esz], esz);
            e.mask = (r + c) % 5 == 4 ? (filters == 2 ? 1u : filters == 1 ? 1u : 0u) : 0u;   // some chunks skip the first filter
            const bool shuffled = filters == 2 && !(e.mask & 1u), deflated = filters >= 1 && !(e.mask & (filters == 2 ? 2u : 1u));
            const uint8_t *src = plain.data();
            if (shuffled) {
                const size_t n = raw / esz;
                for (size_t i = 0; i < n; ++i)
                    for (int b = 0; b < esz; ++b) shuf[(size_t)b * n + i] = plain[i * esz + b];
                src = shuf.data();
            }
            size_t nb = raw;
            if (deflated) {
                uLongf zn = (uLongf)z.size();
                if (compress2(z.data(), &zn, src, (uLong)raw, 2) != Z_OK) return 1;
                nb = zn;
                src = z.data();
                if (truncate && r == 0 && c == 0) nb /= 2;
            }
            if (pwrite(fd, src, nb, (off_t)off) != (ssize_t)nb) return 1;
            e.addr = off; e.size = nb;
            off += nb + 3;
        }
    int bad = 0;
    const int64_t blocks[][2] = {{0, C}, {0, 1}, {C - 1, C}, {C / 3, C / 3 + chc + 1}, {chc, 2 * chc < C ? 2 * chc : C}};
    for (int threads : {1, 4})
        for (auto &b : blocks) {
            const int64_t c0 = b[0], c1 = b[1] < C ? b[1] : C, B = c1 - c0, ldt = B + (threads == 4 ? 3 : 0);
            if (c0 < 0 || c0 >= c1) continue;
            std::vector<uint8_t> tile((size_t)G * ldt * esz, 0xAB);
            int64_t bad_chunk = -2;
            void *calls[4] = {(void *)chunk_size, (void *)read_chunk, nullptr, nullptr};
            const int rc = vcy_loom_block_host(calls, 1, G, C, chr, chc, esz, filters, c0, c1, tile.data(), ldt, threads, &bad_chunk);
            if (truncate) {
                const bool touches = c0 < chc;                            // the cut chunk is chunk 0 of blocks that start in the first column
                if (rc != (touches ? -4 : 0) || (touches && bad_chunk != 0)) { printf("truncated: rc %d chunk %lld\n", rc, (long long)bad_chunk); ++bad; }
                continue;
            }
            if (rc != 0) { printf("rc %d: %s\n", rc, vcy_last_error()); ++bad; continue; }
            for (int64_t g = 0; g < G; ++g) {
                if (memcmp(&tile[(size_t)g * ldt * esz], &full[((size_t)g * C + c0) * esz], (size_t)B * esz)) { ++bad; break; }
                for (size_t p = (size_t)B * esz; p < (size_t)ldt * esz; ++p)
                    if (tile[(size_t)g * ldt * esz + p] != 0xAB) { ++bad; break; }   // the row's padding is not touched
            }
        }
    close(fd);
    if (bad) printf("FAILED esz %d filters %d G %lld C %lld chunk %lld x %lld\n", esz, filters, (long long)G, (long long)C, (long long)chr, (long long)chc);
    return bad;
}

int main()
{
    int bad = 0;
    for (int esz : {1, 2, 4, 8})
        for (int filters : {0, 1, 2}) {
            bad += run(esz, filters, 130, 200, 64, 64, false);
            bad += run(esz, filters, 65, 129, 32, 128, false);
            bad += run(esz, filters, 23, 17, 64, 64, false);
        }
    bad += run(2, 1, 130, 200, 64, 64, true);
    bad += run(4, 2, 130, 200, 64, 64, true);
    printf(bad ? "loom_host_check: %d failures\n" : "loom_host_check: ok\n", bad);
    return bad != 0;
}
