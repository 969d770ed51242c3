"""Python restatement of the rectangular linear-sum-assignment solver ``scipy.optimize.linear_sum_assignment`` runs (shortest
augmenting paths, fp64), with its arithmetic order and its tie-breaking -- the algorithm yogo_amd/csrc/match.hip implements.
``lsap`` scans the remaining columns sequentially as scipy does; ``lsap_par`` writes the scan as the lane-parallel reduction of the
kernel: among the positions whose shortest-path cost equals the minimum, the LAST position whose column is unassigned if there is
one, otherwise the FIRST position.  tests/test_match_host.py holds both to scipy's answer."""
import numpy as np


def lsap(cost):
    cost = np.asarray(cost, dtype=np.float64)
    nr, nc = cost.shape
    transpose = nc < nr
    if transpose:
        cost = np.ascontiguousarray(cost.T)
        nr, nc = nc, nr
    if nr == 0 or nc == 0:
        return np.zeros(0, int), np.zeros(0, int)
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col, path = [-1] * nr, [-1] * nc, [-1] * nc
    INF = float("inf")
    for cur in range(nr):
        minVal, i = 0.0, cur
        remaining = [nc - it - 1 for it in range(nc)]
        num_remaining = nc
        SR, SC = [False] * nr, [False] * nc
        spc = [INF] * nc
        sink = -1
        while sink == -1:
            index, lowest = -1, INF
            SR[i] = True
            for it in range(num_remaining):
                j = remaining[it]
                r = minVal + cost[i, j] - u[i] - v[j]
                if r < spc[j]:
                    path[j], spc[j] = i, r
                if spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1):
                    lowest, index = spc[j], it
            minVal = lowest
            if minVal == INF:
                raise ValueError("cost matrix is infeasible")
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            num_remaining -= 1
            remaining[index] = remaining[num_remaining]
        u[cur] += minVal
        for i2 in range(nr):
            if SR[i2] and i2 != cur:
                u[i2] += minVal - spc[col4row[i2]]
        for j2 in range(nc):
            if SC[j2]:
                v[j2] -= minVal - spc[j2]
        j = sink
        while True:
            i2 = path[j]
            row4col[j] = i2
            col4row[i2], j = j, col4row[i2]
            if i2 == cur:
                break
    if transpose:
        order = np.argsort(col4row, kind="stable")
        return np.array([col4row[k] for k in order]), np.array(order)
    return np.arange(nr), np.array(col4row)


def lsap_par(cost):
    """the same solver with the inner scan as a reduction over all remaining positions at once"""
    cost = np.asarray(cost, dtype=np.float64)
    nr, nc = cost.shape
    transpose = nc < nr
    if transpose:
        cost = np.ascontiguousarray(cost.T)
        nr, nc = nc, nr
    if nr == 0 or nc == 0:
        return np.zeros(0, int), np.zeros(0, int)
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col, path = np.full(nr, -1), np.full(nc, -1), np.full(nc, -1)
    for cur in range(nr):
        minVal, i = 0.0, cur
        remaining, num = np.arange(nc - 1, -1, -1), nc
        spc = np.full(nc, np.inf)
        visited = []                     # the visited columns in order; the visited rows are cur and the rows they were assigned to
        sink = -1
        while sink == -1:
            js = remaining[:num]
            r = ((minVal + cost[i, js]) - u[i]) - v[js]
            upd = r < spc[js]
            path[js[upd]] = i
            spc[js[upd]] = r[upd]
            s = spc[js]
            lowest = s.min()
            if lowest == np.inf:
                raise ValueError("cost matrix is infeasible")
            at = np.nonzero(s == lowest)[0]
            free = at[row4col[js[at]] == -1]
            index = free[-1] if len(free) else at[0]
            j = js[index]
            minVal = spc[j]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            visited.append(j)
            num -= 1
            remaining[index] = remaining[num]
        u[cur] += minVal
        for j in visited:
            d = minVal - spc[j]
            v[j] -= d
            if j != sink:
                u[row4col[j]] += d
        j = sink
        while True:
            i2 = path[j]
            row4col[j] = i2
            col4row[i2], j = j, col4row[i2]
            if i2 == cur:
                break
    if transpose:
        order = np.argsort(col4row, kind="stable")
        return col4row[order], order
    return np.arange(nr), col4row
