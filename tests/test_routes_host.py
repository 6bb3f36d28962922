"""tests/_routes.py on the CPU: the parser reads the line the library prints, and the library holds that line."""
from tests import _routes as routes


def test_route_lines_parse():
    err = ("[nbody] tile walk: 12 terms, estimate counted (shift 0, total 12), 8192 per wave, overflow 0\n"
           "[nbody] walk route: route=tile arm=exact rows=8 srec=1 rec_mode=-1 prep=plain ahead=0 n_tgt=4097 f64=0\n"
           "[nbody] step ahead: build verdict 1 (99 nodes, depth 7, fallback 0, 3 blind levels)\n"
           "[nbody] walk route: route=tile arm=fast-registers rows=-1 srec=-1 rec_mode=3 prep=scan-tail ahead=1 n_tgt=4097 f64=0\n"
           "[nbody] walk route: route=small-leaves arm=none rows=-1 srec=-1 rec_mode=-1 prep=none ahead=0 n_tgt=500 f64=1\n")
    ran = routes.parse(err)
    assert [r.route for r in ran] == [routes.TILE, routes.TILE, routes.SMALL]
    assert ran[1] == routes.Route("tile", "fast-registers", -1, -1, 3, "scan-tail", 1, 4097, 0)
    assert routes.routes(err, ahead=True) == {routes.TILE} and routes.routes(err) == {routes.TILE, routes.SMALL}
    assert routes.kernels(err) == {("exact", 8, 1, -1), ("fast-registers", -1, -1, 3)}


def test_both_libraries_print_the_route_line(nb):
    C = nb._capi
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        with open(path, "rb") as f:
            assert b"[nbody] walk route: route=" in f.read(), path


def test_the_rule_of_the_walk_phase_restated():
    r = routes.expected_bvh_route
    assert r(4095, 64, 1, lab=False) == routes.FUSED and r(4096, 64, 1, lab=False) == routes.TILE
    assert r(500, 16, 3, lab=False) == routes.TILE and r(500, 15, 3, lab=False) == routes.SMALL
    assert r(500, 16, 2, lab=True) == routes.THREE_PASS and r(500, 16, 2, lab=False) == routes.FUSED   # the product reads 2 as 1
    assert r(5000, 16, 2, lab=False) == routes.TILE and r(500, 7, 2, lab=True) == routes.SMALL
    assert r(500, 64, 0, lab=True) == routes.FUSED and r(10 ** 6, 64, 0, lab=False) == routes.FUSED


def test_the_rule_of_the_tile_kernel_restated():
    """Against the tuples test_node_record_fetch_variants_walk_the_same_walk (tests/test_gpu_tree.py) asserts from the trace."""
    k = routes.expected_tile_kernel
    for srec, frec in ((1, 0), (0, 1), (1, 3)):
        assert k(False, True, srec=srec, rec_mode=frec) == ("fast-registers", -1, -1, frec)
        assert k(False, False, srec=srec, rec_mode=frec) == ("exact", 8, srec, -1)
    assert k(False, True, fast_rows=0) == ("fast-registers", -1, -1, 3) and k(False, True, fast_rows=1) == ("fast-rows", 8, 1, -1)
    # the product's four: nothing set
    assert k(False, False) == k(True, False) == ("exact", 8, 1, -1)
    assert k(False, True) == ("fast-registers", -1, -1, 3) and k(True, True) == ("fast-rows", 8, 1, -1)
