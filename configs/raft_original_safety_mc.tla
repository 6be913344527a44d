------------------------ MODULE raft_original_safety_mc ------------------------
\* raftmc-base: thirdparty/raft_original.tla
\*
\* configs/raft_original_mc.tla plus Raft's log- and commit-side safety
\* invariants: the block tlc_membership/raft.tla:969-1099 restated over
\* raft_original's variables (as LogMatching in raft_original_mc.tla restates
\* raft.tla:1017-1021).  raft_original has no dynamic configuration, so Quorum
\* is the spec's static one, and "committed" is what commitIndex covers of a
\* server's own log.  Every definition is total: no index leaves its domain
\* (CommittedLen clamps commitIndex to the log, LeaderCompleteness guards
\* log[l][idx]), so none of them can raise a TLC evaluation error.
\*
\* A cfg lists any of them under INVARIANTS (DESIGN.md §12).  To run this under
\* TLC, place a copy of thirdparty/raft_original.tla named raft.tla next to
\* this file.
\*
\* raft.tla's VotesGrantedInv_false and LeaderCompleteness_false have no
\* counterpart here: their counterexamples need two concurrent leaders and a
\* commit, which on raft_original takes 10 distinct messages (DESIGN.md §12).
EXTENDS raft_original_mc

CommittedLen(i) == IF commitIndex[i] <= Len(log[i]) THEN commitIndex[i] ELSE Len(log[i])
Committed(i)    == SubSeq(log[i], 1, CommittedLen(i))
PrefixOf(s, t)  == Len(s) <= Len(t) /\ SubSeq(t, 1, Len(s)) = s
MaxOrZero(s)    == IF s = {} THEN 0 ELSE Max(s)

CommitWithinLog == \A i \in Server : commitIndex[i] <= Len(log[i])
LeaderVotesQuorum ==                      \* raft.tla:988-993, static Quorum
    \A i \in Server : state[i] = Leader =>
        {j \in Server : currentTerm[j] > currentTerm[i] \/
                        (currentTerm[j] = currentTerm[i] /\ votedFor[j] = i)} \in Quorum
CandidateTermNotInLog ==                  \* raft.tla:997-1004
    \A i \in Server :
        (/\ state[i] = Candidate
         /\ {j \in Server : currentTerm[j] = currentTerm[i] /\ votedFor[j] \in {i, Nil}} \in Quorum) =>
        \A j \in Server : \A n \in DOMAIN log[j] : log[j][n].term /= currentTerm[i]
LeaderHasLatestOfTerm ==                  \* raft.tla:1009-1014 (its "ElectionSafety"; our name is taken)
    \A i \in Server : state[i] = Leader => \A j \in Server :
        MaxOrZero({n \in DOMAIN log[i] : log[i][n].term = currentTerm[i]}) >=
        MaxOrZero({n \in DOMAIN log[j] : log[j][n].term = currentTerm[i]})
VotesGrantedInv ==                        \* raft.tla:1048-1052
    \A i, j \in Server : votedFor[i] = j => PrefixOf(Committed(i), log[j])
QuorumLogInv ==                           \* raft.tla:1056-1060
    \A i \in Server : \A S \in Quorum : \E j \in S : PrefixOf(Committed(i), log[j])
MoreUpToDateCorrect ==                    \* raft.tla:1066-1071
    \A i, j \in Server :
       (\/ LastTerm(log[i]) > LastTerm(log[j])
        \/ /\ LastTerm(log[i]) = LastTerm(log[j]) /\ Len(log[i]) >= Len(log[j])) =>
       PrefixOf(Committed(j), log[i])
LeaderCompleteness ==                     \* raft.tla:1089-1099, guarded
    \A i \in Server : \A idx \in 1..CommittedLen(i) : \A l \in Server :
        (state[l] = Leader /\ currentTerm[l] > log[i][idx].term) =>
        (idx <= Len(log[l]) /\ log[l][idx] = log[i][idx])
StateMachineSafety ==
    \A i, j \in Server :
        \A n \in (1..CommittedLen(i)) \cap (1..CommittedLen(j)) : log[i][n] = log[j][n]
\* test-only control, reachable: every server holds every committed entry
AllHaveCommitted_false == \A i, j \in Server : PrefixOf(Committed(i), log[j])
===============================================================================
