"""The group-row layout of the cross-validated covariance modes (csrc/group_rows.hpp), checked by what the compiled header
does: a stand-alone host program built with g++, no GPU.  driver_direct.cpp predicts the dense group moments pass's grid with
group_row_chunks and covariance.hip launches it from group_rows, both at cov_rows_per_chunk's rows: the layout itself, the
count against the layout in each of the four modes, and the rows per chunk against the numpy restatement the pass tests cut
their chunks by (covariance_passes_reference.rows_per_chunk)."""
import numpy as np

import covariance_passes_reference as ref
from test_direct_plan_host import compile_and_run

PROGRAM = '''#include "group_rows.hpp"
#include <cstdio>
using namespace sgdnet;
template <class V> static void line(const char* name, const V& v) {
  printf("%%s", name);
  for (auto e : v) printf(" %%lld", (long long)e);
  printf("\\n");
}
// the layout at rows_per_chunk rows, and what the count-only form says of the same groups
static void layout(const std::vector<int32_t>& fold, int G, long long rows_per_chunk, long long max_chunks) {
  std::vector<int64_t> count((size_t)G, 0);
  for (int32_t f : fold) ++count[(size_t)f];
  GroupRows r;
  const bool built = group_rows(fold.data(), (int64_t)fold.size(), G, rows_per_chunk, max_chunks, &r);
  printf("built %%d count %%lld chunks %%zu\\n", built ? 1 : 0, (long long)group_row_chunks(count.data(), G, rows_per_chunk), r.chunks());
  line("perm", r.perm);
  line("chunk_begin", r.chunk_begin);
  line("group_chunk", r.group_chunk);
}
int main() {
  const std::vector<int32_t> fold = {%s};
  layout(fold, %d, %d, 65535);
  layout(std::vector<int32_t>(40, 0), 1, 16, 65535);
  layout(fold, %d, %d, 6);
  const std::vector<int32_t> two = {%s};
  for (int wide = 0; wide < 2; ++wide)
    for (int K = 1; K < 3; ++K) layout(two, 2, cov_rows_per_chunk(%d, %d + K + 1, wide != 0), 65535);
%s  return 0;
}
'''

SIZES = (1, 16, 17, 33)
ROWS_PER_CHUNK = 16
MODES_N, MODES_P = 600, 3                        # the four modes: p + K + 1 columns, K = 1 (covariance, wcovariance) and 2
RULE = [(n, ncols, wide) for wide in (False, True) for n in (1, 255, 256, 257, 300, 600, 4097, 10 ** 6)
        for ncols in (2, 5, 16, 17, 200, 513, 724, 725, 4533)]


def interleaved_folds():
    """group g has SIZES[g] rows; the ids go round the groups that still have rows left, so no group's rows are adjacent"""
    left, fold = list(SIZES), []
    while any(left):
        for g in range(len(SIZES)):
            if left[g]:
                left[g] -= 1
                fold.append(g)
    return np.array(fold)


def parse(block):
    head = block[0].split()
    out = dict(built=int(head[1]), count=int(head[3]), chunks=int(head[5]))
    for line in block[1:]:
        name, *values = line.split()
        out[name] = np.array(values, dtype=np.int64)
    return out


def assert_layout(got, fold, G, rows_per_chunk):
    n = len(fold)
    assert got["built"] == 1
    assert np.array_equal(got["perm"], np.argsort(fold, kind="stable"))
    begin, gc = got["chunk_begin"], got["group_chunk"]
    assert begin[0] == 0 and begin[-1] == n and (np.diff(begin) > 0).all() and (np.diff(begin) <= rows_per_chunk).all()
    ends = np.cumsum(np.bincount(fold, minlength=G))
    assert len(gc) == G + 1 and gc[0] == 0 and gc[-1] == len(begin) - 1 == got["chunks"] == got["count"]
    for g in range(G):                                 # a group's chunks tile its rows: none crosses the group's end
        assert begin[gc[g]] == ends[g] - np.sum(fold == g) and begin[gc[g + 1]] == ends[g]
    assert np.array_equal(np.diff(gc), -(-np.bincount(fold, minlength=G) // rows_per_chunk))


def test_group_rows(tmp_path):
    fold = interleaved_folds()
    two = np.random.default_rng(0).permutation(np.repeat([0, 1], [257, MODES_N - 257]))
    rule = "".join('  printf("%%lld\\n", (long long)cov_rows_per_chunk(%dll, %d, %s));\n' % (n, ncols, "true" if wide else "false")
                   for n, ncols, wide in RULE)
    text = PROGRAM % (", ".join(map(str, fold)), len(SIZES), ROWS_PER_CHUNK, len(SIZES), ROWS_PER_CHUNK, ", ".join(map(str, two)),
                      MODES_N, MODES_P, rule)
    lines = compile_and_run(str(tmp_path), "group_rows", text).split("\n")
    blocks = [parse(lines[4 * i:4 * i + 4]) for i in range(7)]

    # sizes {1, 16, 17, 33} at 16 rows a chunk: 1 + 1 + 2 + 3 chunks
    assert_layout(blocks[0], fold, len(SIZES), ROWS_PER_CHUNK)
    assert list(blocks[0]["group_chunk"]) == [0, 1, 2, 4, 7] and blocks[0]["count"] == 7
    assert list(blocks[0]["chunk_begin"]) == [0, 1, 17, 33, 34, 50, 66, 67]
    # one group
    assert_layout(blocks[1], np.zeros(40, dtype=np.int64), 1, ROWS_PER_CHUNK)
    assert list(blocks[1]["group_chunk"]) == [0, 3] and list(blocks[1]["chunk_begin"]) == [0, 16, 32, 40]
    # more chunks than the grid takes: nothing is built, the count says how many there would be
    assert blocks[2]["built"] == 0 and blocks[2]["count"] == 7 and blocks[2]["chunks"] == 0 and len(blocks[2]["perm"]) == 0

    # the four modes at 600 x 3: what the driver counts is what the run lays out, at the rows the pass tests cut by
    for i, (wide, K) in enumerate(((w, K) for w in (False, True) for K in (1, 2))):
        rows = ref.rows_per_chunk(MODES_N, MODES_P + K + 1, wide)
        assert rows == 256
        assert_layout(blocks[3 + i], two, 2, rows)
        assert blocks[3 + i]["count"] == blocks[3 + i]["chunks"] == 4                     # 257 and 343 rows: two chunks each

    # the rows of a chunk, narrow and wide, against the numpy restatement
    got = [int(v) for v in lines[28:28 + len(RULE)]]
    assert got == [ref.rows_per_chunk(n, ncols, wide) for n, ncols, wide in RULE]
