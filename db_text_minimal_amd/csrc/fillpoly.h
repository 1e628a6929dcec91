// cv2.fillPoly(img, [pts], color) with integer vertices, evaluated per pixel in closed form (shared by postproc.hip and
// gtmaps.hip).  A pixel is set if it lies on the 8-connected Bresenham line of an edge (LineIterator, left-to-right) or
// inside the even-odd scanline fill in 16.16 fixed point (OpenCV drawing.cpp: fillPoly -> CollectPolyEdges +
// FillEdgeCollection, Line -> LineIterator; XY_SHIFT = 16).  Coordinates may lie outside the image: the caller asks only
// for the pixels it owns, which is the clipping OpenCV applies.  PARITY UNPINNED against cv2 itself: the tests pin it
// against a CPU restatement of the same published algorithm.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ long long dbn_trunc_div(long long a, long long b) { return a / b; }  // C++: toward zero, like OpenCV

// pixel (px,py) on the 8-connected line from (xa,ya) to (xb,yb)?
__device__ __forceinline__ bool dbn_on_line(int px, int py, int xa, int ya, int xb, int yb) {
    int dx = xb - xa, dy = yb - ya, x1 = xa, y1 = ya;
    if (dx < 0) { x1 = xb; y1 = yb; dx = -dx; dy = -dy; }
    const int sy = dy < 0 ? -1 : 1;
    dy = dy < 0 ? -dy : dy;
    if (dy > dx) {  // steep: one pixel per row
        const int i = (py - y1) * sy;
        if (i < 0 || i > dy) return false;
        const int m = (2 * dx * i + dy - 1) / (2 * dy);
        return px == x1 + m;
    }
    const int i = px - x1;
    if (i < 0 || i > dx) return false;
    const int m = dx == 0 ? 0 : (2 * dy * i + dx - 1) / (2 * dx);
    return py == y1 + sy * m;
}

// is pixel (px,py) set by cv2.fillPoly of the closed polygon (vx[i], vy[i]), i < P?
__device__ __forceinline__ bool dbn_fillpoly_hit(int px, int py, const int* vx, const int* vy, int P) {
    bool in = false;
    int A = 0, B = 0;
    for (int i = 0; i < P; ++i) {
        const int j = i == 0 ? P - 1 : i - 1;
        int xa = vx[j], ya = vy[j], xb = vx[i], yb = vy[i];
        in = in || dbn_on_line(px, py, xa, ya, xb, yb);
        if (ya == yb) continue;
        if (ya > yb) { int t = xa; xa = xb; xb = t; t = ya; ya = yb; yb = t; }
        if (py < ya || py >= yb) continue;
        const long long dxf = dbn_trunc_div((long long)(xb - xa) << 16, (long long)(yb - ya));
        const long long xe = ((long long)xa << 16) + (long long)(py - ya) * dxf;
        A += ((xe + 65535) >> 16) <= px;
        B += (xe >> 16) < px;
    }
    return in || A > B || (B & 1);
}
