#!/usr/bin/env python3
"""Writes the 256-entry byte tables of the colormaps render.py ships, one `<name>.txt` per map with a line `r g b` per
entry: what matplotlib's Colormap.__call__(..., bytes=True) looks up, (lut * 255).astype(uint8).  Run once with matplotlib
installed (the committed tables come from matplotlib 3.10.8); the package itself never imports matplotlib, and
tests/test_render_cpu.py compares the tables with the installed matplotlib."""
import os

import numpy as np
from matplotlib import colormaps

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ('inferno', 'jet')

if __name__ == '__main__':
    for name in NAMES:
        table = colormaps[name](np.arange(256), bytes=True)[:, :3]  # integer input indexes the table
        assert table.shape == (256, 3) and table.dtype == np.uint8
        with open(os.path.join(HERE, name + '.txt'), 'w') as f:
            f.write(''.join('%d %d %d\n' % tuple(int(v) for v in row) for row in table))
