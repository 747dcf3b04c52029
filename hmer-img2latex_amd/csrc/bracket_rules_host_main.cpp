// The bracket constraint's rules (bracket_rules.inc.h) as a stand-alone host program, so that a host test can walk them
// step by step -- depth 32, budgets that run out, broken tables -- under the host sanitizers
// (-fsanitize=address,undefined) in a process of its own.  The walk, and the formats of CASES ("BRKT") and OUT (16 bytes
// of state per step), are rules_walk_host.inc.h's.
//
//   bracket_rules_host_main CASES OUT
#include "rules_walk_host.inc.h"

int main(int argc, char** argv) { return argc == 3 ? walk_cases<BracketModel>(argv[1], argv[2], "BRKT") : 2; }
