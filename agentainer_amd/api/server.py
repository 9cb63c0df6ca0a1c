"""REST API + agent proxy — the reference's HTTP surface, engine-backed.

Route table mirrors `internal/api/server.go:68-107`:

  public:      GET  /health
               ANY  /agent/{id}/{path...}         (unauthenticated proxy)
  authed:      POST /agents                        deploy
               GET  /agents                        list
               GET  /agents/{id}
               POST /agents/{id}/start|stop|restart|pause|resume
               DELETE /agents/{id}                 remove
               GET  /agents/{id}/logs
               POST /agents/{id}/invoke            (real dispatch — the
                                                    reference's stub,
                                                    server.go:407-430, is
                                                    implemented here per
                                                    SURVEY.md §7.4)
               GET  /agents/{id}/metrics, /agents/{id}/metrics/history
               GET  /agents/{id}/requests, /agents/{id}/requests/{reqId}
               POST /agents/{id}/requests/{reqId}/replay
               GET  /agents/{id}/health, /health/agents
  extra (unifying CLI-direct paths per SURVEY.md §1 note):
               POST/GET /backups, POST /backups/{id}/restore,
               DELETE /backups/{id}, GET /audit, GET /logs

Responses use the reference's envelope {success, message, data}
(server.go:50-54). Auth: bearer token or ?token= (server.go:449-478);
per-agent tokens are honored in addition to the server token (fixing the
stored-but-unused Token field). Input caps mirror deploy
validation: name<=64, model<=256, env<=50 entries (server.go:157-179).
"""

from __future__ import annotations

import json
import time
from typing import Any, Dict, Optional

from fastapi import Depends, FastAPI, Header, Query, Request as HttpRequest
from fastapi.responses import JSONResponse, StreamingResponse
from starlette.concurrency import run_in_threadpool

from ..registry import AgentNotFound
from ..engine.base import ModelNotFound
from ..service import Runtime


def envelope(success: bool, message: str = "", data: Any = None) -> Dict[str, Any]:
    return {"success": success, "message": message, "data": data}


def create_app(rt: Runtime) -> FastAPI:
    app = FastAPI(title="agentainer-amd", version="0.1.0")
    app.state.runtime = rt
    server_token = rt.config.get("security", "api_token")

    @app.on_event("startup")
    async def _size_threadpool():
        # every in-flight chat BLOCKS a threadpool worker on done.wait();
        # anyio's default limiter is 40 tokens, which silently caps the
        # server at ~40 concurrent generations (measured: 53 req/s HTTP
        # vs ~200 engine-direct at the same shape). Size it for the
        # multi-hundred-agent regime — a parked thread costs only memory.
        import anyio

        limiter = anyio.to_thread.current_default_thread_limiter()
        limiter.total_tokens = max(
            int(rt.config.get("server", "threadpool_size", 1024)),
            limiter.total_tokens)

    # ---------- auth ----------

    def _client(request: HttpRequest) -> Dict[str, str]:
        return {
            "ip": request.client.host if request.client else "",
            "user_agent": request.headers.get("user-agent", ""),
        }

    async def require_auth(request: HttpRequest,
                           authorization: Optional[str] = Header(None),
                           token: Optional[str] = Query(None)) -> str:
        presented = token
        if authorization and authorization.lower().startswith("bearer "):
            presented = authorization[7:]
        valid = {server_token}
        # per-agent tokens may manage that agent's own routes
        agent_id = request.path_params.get("agent_id")
        if agent_id:
            agent = rt.agents.try_get(agent_id)
            if agent and agent.token:
                valid.add(agent.token)
        if presented not in valid:
            raise AuthError()
        return presented or ""

    class AuthError(Exception):
        pass

    @app.exception_handler(AuthError)
    async def _auth_err(request, exc):
        return JSONResponse(status_code=401,
                            content=envelope(False, "unauthorized"))

    @app.exception_handler(AgentNotFound)
    async def _nf_err(request, exc):
        return JSONResponse(status_code=404, content=envelope(False, str(exc)))

    @app.exception_handler(ModelNotFound)
    async def _model_err(request, exc):
        return JSONResponse(status_code=400, content=envelope(False, str(exc)))

    # ---------- public ----------

    @app.get("/health")
    async def health():
        return envelope(True, "ok", {"status": "healthy", "ts": time.time()})

    @app.api_route("/agent/{agent_id}/{agent_path:path}",
                   methods=["GET", "POST", "PUT", "DELETE", "PATCH"])
    async def proxy(agent_id: str, agent_path: str, request: HttpRequest):
        body: Any = None
        if request.method in ("POST", "PUT", "PATCH"):
            try:
                body = await request.json()
            except Exception:
                raw = await request.body()
                body = {"message": raw.decode("utf-8", "replace")} if raw else {}
        replay = request.headers.get("x-agentainer-replay", "").lower() == "true"
        req_id = request.headers.get("x-agentainer-request-id") or None
        # SSE streaming on the chat path: opt in with {"stream": true},
        # ?stream=1 or Accept: text/event-stream
        wants_stream = (
            agent_path.strip("/") == "chat" and request.method == "POST"
            and not replay
            and (bool(isinstance(body, dict) and body.get("stream"))
                 or request.query_params.get("stream") in ("1", "true")
                 or "text/event-stream" in request.headers.get("accept", "")))
        if wants_stream:
            if isinstance(body, dict):
                body = {k: v for k, v in body.items() if k != "stream"}
            status, result = await run_in_threadpool(
                rt.agent_request_stream, agent_id, body,
                {"content-type": request.headers.get("content-type", "")})
            if status != 200:
                return JSONResponse(status_code=status, content=result)

            def sse():  # sync generator — starlette iterates in threadpool
                for ev in result:
                    yield f"data: {json.dumps(ev)}\n\n"

            return StreamingResponse(sse(), media_type="text/event-stream")
        # blocking dispatch (a generation can take seconds) runs in the
        # threadpool so concurrent requests reach the engine together —
        # that concurrency IS what feeds the continuous-batching scheduler
        status, payload = await run_in_threadpool(
            rt.agent_request, agent_id, request.method, "/" + agent_path,
            body=body,
            headers={"content-type": request.headers.get("content-type", "")},
            replay=replay, req_id=req_id)
        return JSONResponse(status_code=status, content=payload)

    # ---------- management ----------

    @app.post("/agents")
    async def deploy(request: HttpRequest, _tok: str = Depends(require_auth)):
        body = await request.json()
        name = str(body.get("name", ""))
        model = str(body.get("model", body.get("image", "")))
        env = body.get("env_vars", body.get("env", {})) or {}
        # input caps (server.go:157-179)
        if not name or len(name) > 64:
            return JSONResponse(status_code=422,
                                content=envelope(False, "name required, <=64 chars"))
        if not model or len(model) > 256:
            return JSONResponse(status_code=422,
                                content=envelope(False, "model required, <=256 chars"))
        if len(env) > 50:
            return JSONResponse(status_code=422,
                                content=envelope(False, "too many env vars (max 50)"))
        agent = await run_in_threadpool(
            lambda: rt.agents.deploy(
                name=name, model=model,
                dtype=body.get("dtype", "bf16"),
                tp_degree=int(body.get("tp_degree", 1)),
                kv_budget=int(body.get("kv_budget", 0)),
                max_context=int(body.get("max_context", 8192)),
                env=env,
                auto_restart=bool(body.get("auto_restart", False)),
                token=body.get("token"),
                health_check=body.get("health_check"),
                system_prompt=body.get("system_prompt", ""),
                lora=str(body.get("lora") or ""),
                sampling=body.get("sampling") or {},
            ))
        cl = _client(request)
        rt.logger.audit("api", "deploy", agent.id, "success", **cl)
        return envelope(True, f"agent {agent.name} deployed", agent.to_dict())

    @app.get("/agents")
    async def list_agents(_tok: str = Depends(require_auth)):
        rt.reconciler.sync_all()  # sync-before-list (agent.go:393-398)
        return envelope(True, "", [a.to_dict() for a in rt.agents.list()])

    @app.get("/agents/{agent_id}")
    async def get_agent(agent_id: str, _tok: str = Depends(require_auth)):
        rt.reconciler.sync_agent(agent_id)
        return envelope(True, "", rt.agents.get(agent_id).to_dict())

    def _lifecycle(op: str):
        async def handler(agent_id: str, request: HttpRequest,
                          _tok: str = Depends(require_auth)):
            fn = getattr(rt.agents, op)
            try:
                agent = await run_in_threadpool(fn, agent_id)
            except AgentNotFound:
                raise
            except Exception as exc:  # noqa: BLE001
                rt.logger.audit("api", op, agent_id, "failure", details=str(exc),
                                **_client(request))
                return JSONResponse(status_code=409, content=envelope(False, str(exc)))
            rt.reconciler.sync_agent(agent_id)  # quick-sync after op (agent.go:174-178)
            rt.logger.audit("api", op, agent_id, "success", **_client(request))
            return envelope(True, f"agent {op}", agent.to_dict() if agent else None)
        return handler

    app.post("/agents/{agent_id}/start")(_lifecycle("start"))
    app.post("/agents/{agent_id}/stop")(_lifecycle("stop"))
    app.post("/agents/{agent_id}/restart")(_lifecycle("restart"))
    app.post("/agents/{agent_id}/pause")(_lifecycle("pause"))
    app.post("/agents/{agent_id}/resume")(_lifecycle("resume"))

    @app.delete("/agents/{agent_id}")
    async def remove(agent_id: str, request: HttpRequest,
                     _tok: str = Depends(require_auth)):
        # detach + KV teardown can block on the engine step mutex
        await run_in_threadpool(rt.agents.remove, agent_id,
                                request_manager=rt.requests)
        rt.logger.audit("api", "remove", agent_id, "success", **_client(request))
        return envelope(True, "agent removed")

    @app.get("/agents/{agent_id}/logs")
    async def logs(agent_id: str, limit: int = 200, _tok: str = Depends(require_auth)):
        return envelope(True, "", rt.agents.get_logs(agent_id, limit=limit))

    @app.post("/agents/{agent_id}/invoke")
    async def invoke(agent_id: str, request: HttpRequest,
                     _tok: str = Depends(require_auth)):
        """Authenticated dispatch — implemented for real (ref stub, §7.4)."""
        body = await request.json()
        path = body.get("path", "/chat")
        method = body.get("method", "POST")
        status, payload = await run_in_threadpool(
            rt.agent_request, agent_id, method, path, body=body.get("body", body))
        return JSONResponse(status_code=status,
                            content=envelope(status < 400, "", payload))

    # ---------- requests (WAL) ----------

    @app.get("/agents/{agent_id}/requests")
    async def list_requests(agent_id: str, status: str = "",
                            _tok: str = Depends(require_auth)):
        rt.agents.get(agent_id)
        allr = rt.requests.all_requests(agent_id)
        if status:
            allr = {status: allr.get(status, [])}
        return envelope(True, "", {k: [r.to_dict() for r in v] for k, v in allr.items()})

    @app.get("/agents/{agent_id}/requests/{req_id}")
    async def get_request(agent_id: str, req_id: str, _tok: str = Depends(require_auth)):
        r = rt.requests.get(agent_id, req_id)
        if r is None:
            return JSONResponse(status_code=404,
                                content=envelope(False, f"request {req_id} not found"))
        return envelope(True, "", r.to_dict())

    @app.post("/agents/{agent_id}/requests/{req_id}/replay")
    async def replay_request(agent_id: str, req_id: str,
                             _tok: str = Depends(require_auth)):
        r = rt.requests.get(agent_id, req_id)
        if r is None:
            return JSONResponse(status_code=404,
                                content=envelope(False, f"request {req_id} not found"))
        status, payload = await run_in_threadpool(
            rt.agent_request, agent_id, r.method, r.path, body=r.body,
            replay=True, req_id=req_id)
        if status == 200:
            rt.requests.store_response(agent_id, req_id, payload)
        return JSONResponse(status_code=status, content=envelope(status < 400, "", payload))

    # ---------- health / metrics ----------

    @app.get("/agents/{agent_id}/health")
    async def agent_health(agent_id: str, _tok: str = Depends(require_auth)):
        rt.agents.get(agent_id)
        st = rt.health.get_status(agent_id) or rt.health.check_one(agent_id)
        return envelope(True, "", st)

    @app.get("/health/agents")
    async def all_health(_tok: str = Depends(require_auth)):
        return envelope(True, "", rt.health.get_all_statuses())

    @app.get("/agents/{agent_id}/metrics")
    async def agent_metrics(agent_id: str, _tok: str = Depends(require_auth)):
        rt.agents.get(agent_id)
        return envelope(True, "", rt.metrics.get_metrics(agent_id) or {})

    @app.get("/agents/{agent_id}/metrics/history")
    async def metrics_history(agent_id: str, duration_s: float = 3600.0,
                              _tok: str = Depends(require_auth)):
        rt.agents.get(agent_id)
        return envelope(True, "", rt.metrics.get_metrics_history(agent_id, duration_s))

    @app.get("/metrics/device")
    async def device_metrics(_tok: str = Depends(require_auth)):
        # device-level sample (HBM + xGMI) from the 10s metrics loop
        return envelope(True, data=rt.store.get("metrics:current:device") or {})

    @app.get("/metrics/engine")
    async def engine_metrics(_tok: str = Depends(require_auth)):
        return envelope(True, "", rt.engine.stats())

    @app.get("/metrics/prometheus")
    async def prometheus_metrics(_tok: str = Depends(require_auth)):
        """Engine + fleet counters in Prometheus text exposition format
        (scrape-ready; beyond the reference, which had no metrics export)."""
        st = await run_in_threadpool(rt.engine.stats)
        lines = []

        def emit(name, value, labels=None, mtype="gauge", help_=""):
            if not any(ln.startswith(f"# TYPE {name} ") for ln in lines):
                if help_:
                    lines.append(f"# HELP {name} {help_}")
                lines.append(f"# TYPE {name} {mtype}")
            lab = ("{" + ",".join(f'{k}="{v}"' for k, v in labels.items()) + "}"
                   if labels else "")
            lines.append(f"{name}{lab} {value}")

        for model, m in (st.get("models") or {}).items():
            L = {"model": model}
            emit("agentainer_engine_steps_total", m.get("steps", 0), L,
                 "counter", "engine steps executed")
            emit("agentainer_decode_tokens_total", m.get("decode_tokens", 0),
                 L, "counter", "decode tokens sampled")
            emit("agentainer_prefill_tokens_total", m.get("prefill_tokens", 0),
                 L, "counter", "prompt tokens prefilled")
            emit("agentainer_kv_pages_used", m.get("kv_pages_used", 0), L)
            emit("agentainer_kv_pages_free", m.get("kv_pages_free", 0), L)
            emit("agentainer_kv_pages_shared", m.get("kv_pages_shared", 0), L)
            emit("agentainer_running_requests", m.get("running", 0), L)
            emit("agentainer_engine_stuck", int(bool(m.get("stuck"))), L)
        if "hbm_total_bytes" in st:
            emit("agentainer_hbm_free_bytes", st.get("hbm_free_bytes", 0))
            emit("agentainer_hbm_total_bytes", st.get("hbm_total_bytes", 0))
        emit("agentainer_agents_attached", len(st.get("agents") or {}))
        from fastapi.responses import PlainTextResponse
        return PlainTextResponse("\n".join(lines) + "\n",
                                 media_type="text/plain; version=0.0.4")

    # ---------- backups / audit / logs ----------

    @app.post("/backups")
    async def create_backup(request: HttpRequest, _tok: str = Depends(require_auth)):
        body = await request.json()
        b = await run_in_threadpool(
            rt.backups.create, body.get("name", "backup"),
            body.get("description", ""), body.get("agent_ids"))
        rt.logger.audit("api", "backup.create", b["id"], "success", **_client(request))
        return envelope(True, "", {"id": b["id"], "n_agents": len(b["agents"])})

    @app.get("/backups")
    async def list_backups(_tok: str = Depends(require_auth)):
        return envelope(True, "", rt.backups.list())

    @app.post("/backups/{backup_id}/restore")
    async def restore_backup(backup_id: str, request: HttpRequest,
                             _tok: str = Depends(require_auth)):
        agents = await run_in_threadpool(rt.backups.restore, backup_id)
        rt.logger.audit("api", "backup.restore", backup_id, "success", **_client(request))
        return envelope(True, "", [a.to_dict() for a in agents])

    @app.delete("/backups/{backup_id}")
    async def delete_backup(backup_id: str, _tok: str = Depends(require_auth)):
        rt.backups.delete(backup_id)
        return envelope(True, "backup deleted")

    @app.get("/backups/{backup_id}/export")
    async def export_backup(backup_id: str, _tok: str = Depends(require_auth)):
        import tempfile

        from fastapi.responses import FileResponse

        out = tempfile.mktemp(suffix=".tar.gz")
        rt.backups.export(backup_id, out)
        return FileResponse(out, filename=f"{backup_id}.tar.gz",
                            media_type="application/gzip")

    @app.post("/backups/import")
    async def import_backup(request: HttpRequest,
                            _tok: str = Depends(require_auth)):
        import tempfile

        raw = await request.body()
        tmp = tempfile.mktemp(suffix=".tar.gz")
        with open(tmp, "wb") as f:
            f.write(raw)
        ids = rt.backups.import_(tmp)
        return envelope(True, "", {"imported": ids})

    @app.get("/audit")
    async def audit_logs(user: str = "", action: str = "", resource: str = "",
                         limit: int = 200, _tok: str = Depends(require_auth)):
        return envelope(True, "", rt.logger.get_audit_logs(
            user=user, action=action, resource=resource, limit=limit))

    @app.get("/logs")
    async def server_logs(level: str = "", component: str = "", agent_id: str = "",
                          limit: int = 200, _tok: str = Depends(require_auth)):
        return envelope(True, "", rt.logger.get_logs(
            level=level, component=component, agent_id=agent_id, limit=limit))

    @app.get("/logs/stream")
    async def logs_stream(agent_id: str = "",
                          _tok: str = Depends(require_auth)):
        """Live log tail over SSE (the reference's TailLogs published to a
        channel nobody could subscribe to — here the stream is usable:
        `agentainer logs -f`). Optional ?agent_id= filter."""
        import queue as _q

        def sse():  # sync generator — starlette iterates in a threadpool
            lines: "_q.Queue[str]" = _q.Queue(maxsize=1000)

            def on_line(line: str) -> None:
                try:
                    lines.put_nowait(line)
                except _q.Full:
                    pass  # slow client: drop rather than block the logger

            unsub = rt.logger.tail(on_line)
            try:
                while True:
                    try:
                        line = lines.get(timeout=15.0)
                    except _q.Empty:
                        yield ": heartbeat\n\n"
                        continue
                    if agent_id:
                        try:
                            if json.loads(line).get("agent_id") != agent_id:
                                continue
                        except json.JSONDecodeError:
                            continue
                    yield f"data: {line}\n\n"
            finally:
                unsub()

        return StreamingResponse(sse(), media_type="text/event-stream")

    return app


def run_server(rt: Runtime, host: Optional[str] = None, port: Optional[int] = None):
    import sys

    import uvicorn

    # The engine thread shares the GIL with every request thread; at the
    # default 5 ms switch interval a ready engine step waits out multiple
    # request-thread slices (measured: 26.7 ms/step under 64-agent HTTP
    # load vs 9.5 ms engine-direct at full batch occupancy). Shorter
    # slices hand the GIL back to the scheduler promptly.
    sys.setswitchinterval(float(rt.config.get("server",
                                              "gil_switch_interval_s", 0.001)))
    app = create_app(rt)
    rt.start_workers()
    rt.recover()
    try:
        uvicorn.run(app,
                    host=host or rt.config.get("server", "host"),
                    port=int(port or rt.config.get("server", "port")),
                    log_level="warning")
    finally:
        rt.shutdown()
