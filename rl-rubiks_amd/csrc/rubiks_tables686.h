// Compile-time tables of the 6x8x6 representation (reference librubiks/cube/cube.py:67-71,311-388): the sticker
// permutation of every action and the bridge from the 20x24 codes to sticker colours.
//
// Nothing here is a move table of its own: both tables are DERIVED from what the project already has --
//   * where each cubie position's stickers sit on the 6x3x3 net and which colours a cubie carries: the sticker layout
//     behind as633 (librubiks/cube/maps.py get_633maps, librubiks/cube/cube.py as633), restated below as kCornerCells /
//     kEdgeCells;
//   * how a 6x8x6 face numbers its 8 stickers: a ring around the centre of the 3x3 face (kRingCell), entered at a
//     face-specific offset (kRingStart) -- the format's definition, which the reference's as633 for this representation
//     reads backwards (cube.py:383-388);
//   * the 20x24 move table kTables.lut.
// bridge[i][v] paints cubie i with code v onto the net; perm[a] follows every (cubie, code) through lut[a] and records
// which sticker each of its colours came from.
#pragma once
#include "rubiks_tables.h"

namespace rubiks {

constexpr int kStickers = 48;   // plane f*8+p = sticker p of face f, colour 0..5
constexpr int kColours = 6;
constexpr int kOh686 = kStickers * kColours;   // one-hot index (f*8+p)*6 + colour
constexpr uint8_t kNoSticker = 0xff;

struct Cell { int8_t face, row, col; };
// F, B, T, D, L, R = 0..5; the first cell of a cubie position is also the colour the cubie's orientation is tracked by
constexpr Cell kCornerCells[8][3] = {
    {{0, 0, 0}, {4, 0, 2}, {2, 2, 0}}, {{0, 2, 0}, {3, 0, 0}, {4, 2, 2}}, {{0, 2, 2}, {5, 2, 0}, {3, 0, 2}}, {{0, 0, 2}, {2, 2, 2}, {5, 0, 0}},
    {{1, 0, 2}, {2, 0, 0}, {4, 0, 0}}, {{1, 2, 2}, {4, 2, 0}, {3, 2, 0}}, {{1, 2, 0}, {3, 2, 2}, {5, 2, 2}}, {{1, 0, 0}, {5, 0, 2}, {2, 0, 2}},
};
constexpr Cell kEdgeCells[12][2] = {
    {{0, 0, 1}, {2, 2, 1}}, {{0, 1, 0}, {4, 1, 2}}, {{0, 2, 1}, {3, 0, 1}}, {{0, 1, 2}, {5, 1, 0}}, {{2, 1, 0}, {4, 0, 1}}, {{3, 1, 0}, {4, 2, 1}},
    {{3, 1, 2}, {5, 2, 1}}, {{2, 1, 2}, {5, 0, 1}}, {{1, 0, 1}, {2, 0, 1}}, {{1, 1, 2}, {4, 1, 0}}, {{1, 2, 1}, {3, 2, 1}}, {{1, 1, 0}, {5, 1, 2}},
};
// ring position k -> 3*row + col: down the first column, along the bottom row, up the last column, back along the top
constexpr int kRingCell[8] = {0, 3, 6, 7, 8, 5, 2, 1};
// sticker p of face f sits at ring position (p - kRingStart[f]) mod 8
constexpr int kRingStart[6] = {0, 6, 6, 4, 2, 4};

constexpr int sticker_of(const Cell &c) {
    const int cell = 3 * c.row + c.col;
    for (int k = 0; k < 8; ++k)
        if (kRingCell[k] == cell) return c.face * 8 + (k + kRingStart[c.face]) % 8;
    return -1;   // a centre: no cubie cell is one
}

struct Tables686 {
    // out sticker s of a cube after action a = in sticker perm[a][s]; rows a >= 12 are identity padding
    uint8_t perm[kActionPad][kStickers];
    // cubie i with code v paints colour bridge[i][v][k][1] on sticker bridge[i][v][k][0], k < 3 (corner) / 2 (edge);
    // unused entries (the third pair of an edge, codes >= 24) have sticker kNoSticker
    uint8_t bridge[kPlanes][kCodePad][3][2];
};

constexpr Tables686 make_tables686() {
    Tables686 t{};
    for (int a = 0; a < kActionPad; ++a)
        for (int s = 0; s < kStickers; ++s) t.perm[a][s] = (uint8_t)s;
    for (int i = 0; i < kPlanes; ++i)
        for (int v = 0; v < kCodePad; ++v)
            for (int k = 0; k < 3; ++k) t.bridge[i][v][k][0] = kNoSticker, t.bridge[i][v][k][1] = 0;
    for (int i = 0; i < kCorners; ++i)
        for (int v = 0; v < kCodes; ++v) {
            const int pos = v / 3, ori = v % 3;
            // positions 0, 2, 5, 7 list their cells with the other handedness (as633: the roll changes sign there)
            const int shift = (pos == 0 || pos == 2 || pos == 5 || pos == 7) ? 3 - ori : ori;
            for (int k = 0; k < 3; ++k) {
                t.bridge[i][v][k][0] = (uint8_t)sticker_of(kCornerCells[pos][k]);
                t.bridge[i][v][k][1] = (uint8_t)kCornerCells[i][(k + 3 - shift % 3) % 3].face;
            }
        }
    for (int i = 0; i < 12; ++i)
        for (int v = 0; v < kCodes; ++v) {
            const int pos = v / 2, ori = v % 2;
            for (int k = 0; k < 2; ++k) {
                t.bridge[kCorners + i][v][k][0] = (uint8_t)sticker_of(kEdgeCells[pos][k]);
                t.bridge[kCorners + i][v][k][1] = (uint8_t)kEdgeCells[i][(k + 2 - ori) % 2].face;
            }
        }
    // action a takes cubie i from code v to code w = lut[a][kind][v]: each of its colours moves from the sticker it had under v
    // to the sticker it has under w (a cubie's colours are distinct, so the colour names the sticker)
    for (int a = 0; a < kActions; ++a)
        for (int i = 0; i < kPlanes; ++i)
            for (int v = 0; v < kCodes; ++v) {
                const int w = kTables.lut[a][i >= kCorners ? 1 : 0][v];
                for (int k = 0; k < 3; ++k) {
                    if (t.bridge[i][v][k][0] == kNoSticker) continue;
                    for (int k2 = 0; k2 < 3; ++k2)
                        if (t.bridge[i][w][k2][0] != kNoSticker && t.bridge[i][w][k2][1] == t.bridge[i][v][k][1])
                            t.perm[a][t.bridge[i][w][k2][0]] = t.bridge[i][v][k][0];
                }
            }
    return t;
}

constexpr Tables686 kTables686 = make_tables686();

}  // namespace rubiks
