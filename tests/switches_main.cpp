// switches_main.cpp -- lws_amd/csrc/lws_switches.h on its own (tests/test_switches.py runs this under environments of its choice).
//   switches_main --table   every row of the table: name kind default when
//   switches_main           the snapshot read_switches() takes of this process's environment: name value
#include <cstdio>
#include <cstring>

#include "../lws_amd/csrc/lws_switches.h"

// (LWS_HOST_THREADS has no constant default: "unset")
static void show(int v) {
    if (v == lws::SWITCH_UNSET) printf("unset");
    else printf("%d", v);
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--table")) {
        for (const lws::SwitchRow &r : lws::switch_rows) {
            printf("%s %s ", r.name, r.kind == lws::SwitchKind::FLAG ? "FLAG" : "INT");
            show(r.dflt);
            printf(" %s\n", r.when == lws::SwitchWhen::CREATE ? "CREATE" : "CALL");
        }
        return 0;
    }
    const lws::Switches s = lws::read_switches();
#define PRINT(field, name, kind, dflt, when) printf("%s ", name), show((int)s.field), printf("\n");
    LWS_SWITCHES(PRINT)
#undef PRINT
    return 0;
}
