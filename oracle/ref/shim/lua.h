/* Stand-in for <lua.h> / luaT.h, for compiling the reference's extras/stnbhwd/BilinearSamplerBHWD.cu outside Torch7
 * (oracle/reference.py).  It declares only the names that file uses.  A lua_State here is a row of argument slots:
 * the driver (oracle/ref/ref_sampler.cpp) fills slot i with the tensor the Lua side would have passed as argument i. */
#ifndef B2F_REF_SHIM_LUA_H
#define B2F_REF_SHIM_LUA_H

#include <cstddef>
#include <cstdio>

#define B2F_REF_SLOTS 8

struct lua_State {
    void *slot[B2F_REF_SLOTS];
};

typedef int (*lua_CFunction)(lua_State *L);

struct luaL_Reg {
    const char *name;
    lua_CFunction func;
};

static inline void *luaT_checkudata(lua_State *L, int i, const char *tname)
{
    (void)tname;
    return L->slot[i];
}

static inline void luaT_pushmetatable(lua_State *L, const char *tname) { (void)L; (void)tname; }
static inline void luaT_registeratname(lua_State *L, const struct luaL_Reg *methods, const char *name) { (void)L; (void)methods; (void)name; }
static inline void lua_pop(lua_State *L, int n) { (void)L; (void)n; }

#endif
