--------------------- MODULE raft_original_actions_sym_mc ----------------------
\* raftmc-base: thirdparty/raft_original.tla
\*
\* configs/raft_original_actions_mc.tla plus the symmetry set of
\* configs/raft_original_sym_mc.tla: every action property quantifies over all
\* of Server and names no server (Restart(i) has i bound), so its truth on a
\* step is unchanged by a permutation of Server applied to both states, and a
\* cfg may list it together with
\*     SYMMETRY ServerSymmetry
\* (DESIGN.md §11, §14).  To run this under TLC, place a copy of
\* thirdparty/raft_original.tla named raft.tla next to this file.
EXTENDS raft_original_actions_mc, TLC

ServerSymmetry == Permutations(Server)
===============================================================================
