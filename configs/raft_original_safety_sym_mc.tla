---------------------- MODULE raft_original_safety_sym_mc ----------------------
\* raftmc-base: thirdparty/raft_original.tla
\*
\* configs/raft_original_safety_mc.tla plus the symmetry set of
\* configs/raft_original_sym_mc.tla: every safety invariant quantifies over all
\* of Server and names no server, so it is invariant under a permutation of
\* Server and a cfg may list it together with
\*     SYMMETRY ServerSymmetry
\* (DESIGN.md §11, §12).  To run this under TLC, place a copy of
\* thirdparty/raft_original.tla named raft.tla next to this file.
EXTENDS raft_original_safety_mc, TLC

ServerSymmetry == Permutations(Server)
===============================================================================
