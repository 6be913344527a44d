----------------------- MODULE raft_original_actions_mc ------------------------
\* raftmc-base: thirdparty/raft_original.tla
\*
\* configs/raft_original_safety_mc.tla plus Raft's guarantees that are
\* properties of a step, not of a state: each is an action property
\* [][A]_vars, which TLC checks on every transition it generates (no liveness
\* machinery).  A cfg lists any of them under PROPERTIES (DESIGN.md §14).
\*
\*   TermsMonotonic        terms never go back
\*   OneVotePerTerm        at most one vote per term: within a term a vote,
\*                         once given, is neither withdrawn nor changed
\*   LeaderAppendOnly      a leader only appends to its log (Raft paper, Fig. 3)
\*   CommittedNeverLost    a committed entry is never dropped from the log that
\*                         held it
\*   CommitIndexMonotonic  commitIndex only goes back when the server restarts.
\*                         raft_original.tla:360-362 says of
\*                         commitIndex' = m.mcommitIndex: "This could make our
\*                         commitIndex decrease (for example if we process an
\*                         old, duplicated request), but that doesn't really
\*                         affect anything."  This property shows that
\*                         behaviour: it FAILS on configs/pair7_commit_regress.cfg.
\*
\* To run this under TLC, place a copy of thirdparty/raft_original.tla named
\* raft.tla next to this file.
EXTENDS raft_original_safety_mc

TermsMonotonic       == [][\A i \in Server : currentTerm'[i] >= currentTerm[i]]_vars
OneVotePerTerm       == [][\A i \in Server : (currentTerm'[i] = currentTerm[i] /\ votedFor[i] /= Nil)
                                              => votedFor'[i] = votedFor[i]]_vars
LeaderAppendOnly     == [][\A i \in Server : (state[i] = Leader /\ state'[i] = Leader)
                                              => PrefixOf(log[i], log'[i])]_vars
CommittedNeverLost   == [][\A i \in Server : PrefixOf(Committed(i), log'[i])]_vars
CommitIndexMonotonic == [][\A i \in Server : commitIndex'[i] >= commitIndex[i] \/ Restart(i)]_vars
\* test-only control, reachable as soon as a leader restarts or sees a newer term
LeaderNeverStepsDown_false == [][\A i \in Server : state[i] = Leader => state'[i] = Leader]_vars
===============================================================================
