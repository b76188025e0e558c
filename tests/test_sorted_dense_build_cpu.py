"""CPU checks of the sorted dense join build (no GPU): the catalog's generated build modules carry its entry point beside the
atomic one, for a host-side and a device-side build row count, and the key policy tells NULL keys from filtered rows."""
from qurious_amd import catalog


def test_q3_dense_build_sources_hold_the_sorted_entry_point():
    srcs = dict(catalog.catalog_sources())
    db, db_dr = srcs["q3 join-1 output dense build"], srcs["q3 join-1 output dense build, device-side row count"]
    for src in (db, db_dr):
        assert "qk_join_dense_build(" in src and "qk_join_dense_build_sorted(" in src
        assert "static __forceinline__ u32 key_state(" in src
    assert "qh_join_dense_build_sorted_body<P>" in db and "qh_join_dense_build_sorted_body<P, true>" in db_dr
    # join 1's build side (customer, fused Utf8 scan filter): the row_of form needs the filter apart from the key
    cust = srcs["q3 customer dense build"]
    assert "qk_join_dense_build_sorted(" in cust and "qh_streq_lit" in cust
