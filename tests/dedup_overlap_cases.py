"""The case names tests/native/orig_dedup_overlap_check.hip must report (one JSON line each)."""

OVERLAP_CASES = (["overlap_records_%d" % n for n in (0, 1, 511, 512, 513)] +
                 ["overlap_lds_window_wraps", "overlap_duplicates", "overlap_table_cluster_wraps"])
