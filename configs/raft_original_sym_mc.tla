------------------------- MODULE raft_original_sym_mc -------------------------
\* raftmc-base: thirdparty/raft_original.tla
\*
\* configs/raft_original_mc.tla plus a symmetry set: raft_original.tla treats
\* servers interchangeably (Init, every action and every operator of the MC
\* wrapper are invariant under a permutation of Server), so a cfg may declare
\*     SYMMETRY ServerSymmetry
\* and the search keeps one state per orbit (DESIGN.md §11).  Value is not
\* declared symmetric.  To run this under TLC, place a copy of
\* thirdparty/raft_original.tla named raft.tla next to this file.
EXTENDS raft_original_mc, TLC

ServerSymmetry == Permutations(Server)
===============================================================================
