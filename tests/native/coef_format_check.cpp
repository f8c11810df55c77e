// Host check of the narrow block form (csrc/coef_format.hpp, the header the
// kernels include): the byte map, the escape, the round trip of every int16 at
// every position, and the rule that picks the form of a call.
// usage: coef_format_check luma_hex chroma_hex   (64 bytes each, natural order, as
// hex) prints the rule for sample sizes 1, 2, 4 under auto / wide / narrow;
// with no argument it runs the checks and prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../dmmt-jpeg-encoder_amd/csrc/coef_format.hpp"

using namespace dmmt;

static int fails = 0;
#define CHECK(c, ...)                \
    do {                             \
        if (!(c)) {                  \
            if (++fails < 20) {      \
                printf("FAIL: ");    \
                printf(__VA_ARGS__); \
                printf("\n");        \
            }                        \
        }                            \
    } while (0)

static int hexval(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

int main(int argc, char** argv) {
    if (argc == 3) {
        uint8_t q[2][64];
        for (int t = 0; t < 2; ++t) {
            if (strlen(argv[1 + t]) != 128) return 2;
            for (int i = 0; i < 64; ++i) q[t][i] = (uint8_t)(hexval(argv[1 + t][2 * i]) * 16 + hexval(argv[1 + t][2 * i + 1]));
        }
        const int sbs[3] = {1, 2, 4};
        for (int sb : sbs)
            printf("sb%d auto=%d wide=%d narrow=%d\n", sb, (int)coef_narrow_for(COEF_FORMAT_AUTO, sb, q[0], q[1]),
                   (int)coef_narrow_for(COEF_FORMAT_WIDE, sb, q[0], q[1]),
                   (int)coef_narrow_for(COEF_FORMAT_NARROW, sb, q[0], q[1]));
        return 0;
    }

    // the byte map: lo positions 0..7 and hi bytes coef_pos(8..63) are a bijection
    // with coef_pos; the bytes of the lo positions are the first coef_lo_rows(c)
    // of column c
    {
        bool seen[64] = {false};
        for (int k = 0; k < 64; ++k) {
            const int p = coef_pos(k);
            CHECK(p >= 0 && p < 64 && !seen[p], "coef_pos(%d) = %d repeats", k, p);
            seen[p] = true;
            CHECK(coef_hi_word(k) * 4 + coef_hi_shift(k) / 8 == p, "word/shift of %d", k);
            const int col = p >> 3, row = p & 7;
            CHECK(coef_in_lo(k) == (row < coef_lo_rows(col)), "lo rows: k %d col %d row %d", k, col, row);
            CHECK(coef_in_lo(k) == (k < 8), "split at %d", k);
        }
        int nlo = 0;
        for (int c = 0; c < 8; ++c) nlo += coef_lo_rows(c);
        CHECK(nlo == kCoefLoCount, "lo count %d", nlo);
        static const int nat[8][2] = {{0, 0}, {0, 1}, {1, 0}, {2, 0}, {1, 1}, {0, 2}, {0, 3}, {1, 2}};
        for (int k = 0; k < 8; ++k) CHECK(kZigzag[k] == nat[k][0] * 8 + nat[k][1], "natural index of zigzag %d", k);
    }

    // every int16 at every position: the stored byte, the escape, the read back.
    // The wide store starts as garbage: only what the pack wrote may be read.
    for (int k = 0; k < 64; ++k) {
        for (int v = -32768; v <= 32767; ++v) {
            int16_t zz[64], lo[8], wide[64];
            int8_t hi[64];
            for (int i = 0; i < 64; ++i) zz[i] = (int16_t)((i * 37 + k) % 255 - 127), wide[i] = 0x5A5A;  // no other escape
            memset(lo, 0x33, sizeof lo);
            memset(hi, 0x33, sizeof hi);
            zz[k] = (int16_t)v;
            coef_pack_block(zz, lo, hi, wide);
            const bool esc = k >= 8 && (v > 127 || v < -127);
            const uint8_t byte = (uint8_t)hi[coef_pos(k)];
            CHECK((byte == 0x80) == esc, "escape byte: k %d v %d byte %02x", k, v, byte);
            if (k < 8 && k > 0) CHECK(byte == 0, "lo position's hi byte: k %d byte %02x", k, byte);
            // position 0's byte is the block's flag
            CHECK((uint8_t)hi[coef_pos(0)] == (esc ? 1 : 0) && coef_block_flag(hi) == esc, "flag: k %d v %d", k, v);
            if (k >= 8 && !esc) CHECK((int8_t)byte == v, "hi byte: k %d v %d", k, v);
            for (int i = 0; i < 64; ++i) {
                const int r = coef_read(i, lo, hi, wide);
                if (r != zz[i]) {
                    CHECK(false, "read back: k %d v %d position %d gives %d", k, v, i, r);
                    break;
                }
            }
            // the wide store is touched only in the escape's column
            for (int i = 0; i < 64; ++i) {
                const bool in_col = esc && (i >> 3) == (coef_pos(k) >> 3);
                if ((wide[i] != 0x5A5A) && !in_col) {
                    CHECK(false, "wide store touched: k %d v %d index %d", k, v, i);
                    break;
                }
            }
        }
    }
    // the byte rule is v_med3_i32(v, -128, 128) & 0xFF
    for (int v = -32768; v <= 32767; ++v) {
        const int m = v < -128 ? -128 : v > 128 ? 128 : v;
        CHECK((uint8_t)m == (uint8_t)coef_hi_byte(v), "med3 form at %d", v);
    }
    if (fails) {
        printf("FAIL: %d checks\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
